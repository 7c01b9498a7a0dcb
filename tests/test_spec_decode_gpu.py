"""Speculative decoding on the GPU: the gfx950 multi-query paged decode
kernel (ops/csrc/attention_verify.hip) against its fp32 reference, its
host checks and graph capture, then Transformer.verify and the engine's
speculative step built on it."""
import dataclasses

import pytest
import torch

from runbooks_amd import ops
from runbooks_amd.models import build_model, get_config
from runbooks_amd.models.transformer import fuse_for_inference
from runbooks_amd.serve import Engine, NgramDrafter

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BS = ops.BLOCK_SIZE
NAN = float("nan")
TOL = 3e-2          # the project's bound for randn data in the paged tests

# (Hq, Hkv, dh, transposed-V, T, [(seq_len, q_len) per sequence])
SHAPES = [
    (4, 4, 128, False, 5, [(5, 5), (17, 1), (64, 3), (300, 5), (9, 0)]),
    (8, 2, 128, True, 4, [(4, 4), (33, 2), (272, 4)]),
    (8, 1, 64, True, 8, [(8, 8), (100, 8), (16, 1)]),
    (6, 2, 128, False, 2, [(2, 2), (49, 1)]),
    (2, 2, 64, False, 1, [(1, 1), (31, 1)]),
]


def _fill(Hq, Hkv, dh, vt, T, seqs, seed, kc=None, vc=None, pool=None):
    """Scattered block pool with randn K/V for each sequence; everything
    the kernel must not read is NaN: the tail of each last block, and a
    spare block behind every unused table entry and the whole table row of
    a q_len = 0 sequence. Returns q, caches, table, seq_lens, q_lens (on the
    device) and the spare block id."""
    g = torch.Generator().manual_seed(seed)
    B = len(seqs)
    nbs = [(s + BS - 1) // BS if n > 0 else 0 for s, n in seqs]
    if kc is None:
        pool = sum(nbs) + 4
        kc, vc = ops.alloc_kv_cache(pool, Hkv, dh, DEV, v_transposed=vt)
    assert ops.attention._is_vt(kc, vc) == vt
    perm = torch.randperm(pool, generator=g).tolist()
    spare = perm.pop()
    maxb = max(nbs) + 2
    table = torch.full((B, maxb), spare, dtype=torch.int32)
    for b, (S, n) in enumerate(seqs):
        if n == 0:
            continue
        blocks = [perm.pop() for _ in range(nbs[b])]
        table[b, :nbs[b]] = torch.tensor(blocks, dtype=torch.int32)
        k = torch.randn(S, Hkv, dh, generator=g).to(torch.bfloat16).to(DEV)
        v = torch.randn(S, Hkv, dh, generator=g).to(torch.bfloat16).to(DEV)
        pos = torch.arange(S)
        slots = (table[b][pos // BS].long() * BS + pos % BS).to(torch.int32)
        ops.kv_append(k, v, kc, vc, slots.to(DEV))
        last, off = blocks[-1], S % BS
        if off:
            kc[last, :, off:, :] = NAN
            if vt:
                vc[last, :, :, off:] = NAN
            else:
                vc[last, :, off:, :] = NAN
    kc[spare] = NAN
    vc[spare] = NAN
    q = torch.randn(B, T, Hq, dh, generator=g).to(torch.bfloat16).to(DEV)
    sl = torch.tensor([s for s, _ in seqs], dtype=torch.int32, device=DEV)
    ql = torch.tensor([n for _, n in seqs], dtype=torch.int32, device=DEV)
    return q, kc, vc, table.to(DEV), sl, ql


def _check(out, q, kc, vc, table, sl, ql, what):
    ref = ops.paged_verify_ref(q.cpu().float(), kc.cpu().float(),
                               vc.cpu().float(), table.cpu(), sl.cpu(),
                               ql.cpu())
    o = out.cpu().float()
    assert not torch.isnan(o).any(), f"{what}: stale cache contents leaked"
    for b in range(q.shape[0]):
        assert (o[b, int(ql[b]):] == 0).all(), f"{what}: padding rows of {b}"
    diff = (o - ref).abs().max().item()
    print(f"{what}: max abs diff vs fp32 ref {diff:.3e}")
    assert diff < TOL, f"{what}: max diff {diff}"


@pytest.mark.parametrize("nsplit", [1, 4])
@pytest.mark.parametrize("Hq,Hkv,dh,vt,T,seqs", SHAPES)
def test_paged_verify_kernel(Hq, Hkv, dh, vt, T, seqs, nsplit):
    assert ops.has_hip()
    q, kc, vc, table, sl, ql = _fill(Hq, Hkv, dh, vt, T, seqs,
                                     seed=dh + 7 * T + Hq)
    out = ops.paged_verify(q, kc, vc, table, sl, ql, nsplit=nsplit)
    torch.cuda.synchronize()
    assert out.shape == q.shape and out.dtype == torch.bfloat16
    _check(out, q, kc, vc, table, sl, ql,
           f"paged_verify dh={dh} vt={vt} T={T} nsplit={nsplit} {seqs}")
    if T == 1:
        dec = ops.paged_decode(q[:, 0].contiguous(), kc, vc, table, sl)
        diff = (out[:, 0].float() - dec.float()).abs().max().item()
        print(f"  T=1 vs paged_decode: max abs diff {diff:.3e}")
        assert diff < TOL


def test_paged_verify_auto_nsplit():
    """nsplit=None picks a split from host-known sizes and meets the same
    bound."""
    Hq, Hkv, dh, vt, T, seqs = SHAPES[1]
    q, kc, vc, table, sl, ql = _fill(Hq, Hkv, dh, vt, T, seqs, seed=3)
    out = ops.paged_verify(q, kc, vc, table, sl, ql)
    torch.cuda.synchronize()
    _check(out, q, kc, vc, table, sl, ql, "paged_verify nsplit=None")


def test_paged_verify_host_checks():
    """Unsupported calls fail on the host, through the public op and
    through the extension entry point itself."""
    assert ops.has_hip()
    ext = ops.ext()
    i32 = dict(dtype=torch.int32, device=DEV)

    def args(B=2, T=3, Hq=2, Hkv=2, dh=64, fp8=False, rows=None):
        kc, vc = ops.alloc_kv_cache(4, Hkv, dh, DEV, fp8=fp8)
        q = torch.zeros(B, T, Hq, dh, dtype=torch.bfloat16, device=DEV)
        bt = torch.zeros(B if rows is None else rows, 3, **i32)
        sl = torch.full((B,), T, **i32)
        ql = torch.full((B,), T, **i32)
        return [q, kc, vc, bt, sl, ql]

    ok = args()
    assert ops.paged_verify(*ok).shape == ok[0].shape
    assert ext.paged_verify(*ok, 1, 0.125).shape == ok[0].shape

    def both(a):
        with pytest.raises((ValueError, TypeError, NotImplementedError,
                            RuntimeError)):
            ops.paged_verify(*a)
        with pytest.raises(RuntimeError):
            ext.paged_verify(*a, 1, 0.125)

    both(args(fp8=True))                     # fp8 cache
    both(args(dh=256))                       # Dh 256
    both(args(T=9))                          # T 9
    both(args(rows=1))                       # table with fewer rows than B
    bad = args()
    bad[5] = bad[5].long()                   # non-int32 q_lens
    both(bad)
    torch.cuda.synchronize()


def test_paged_verify_graph_capture():
    """One captured launch (nsplit=2) serves other lengths, tables and
    queries written into its static tensors between replays."""
    assert ops.has_hip()
    Hq, Hkv, dh, vt, T = 8, 2, 128, True, 4
    cases = [[(40, 4), (7, 2), (130, 1)],
             [(3, 3), (90, 4), (20, 0)],
             [(64, 1), (65, 4), (16, 4)]]
    pool = 40
    kc, vc = ops.alloc_kv_cache(pool, Hkv, dh, DEV, v_transposed=vt)
    q, _, _, table, sl, ql = _fill(Hq, Hkv, dh, vt, T, cases[0], 1, kc, vc,
                                   pool)
    wide = torch.zeros(3, 12, dtype=torch.int32, device=DEV)
    wide[:, :table.shape[1]] = table
    table = wide
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.paged_verify(q, kc, vc, table, sl, ql, nsplit=2)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.paged_verify(q, kc, vc, table, sl, ql, nsplit=2)
    for i, seqs in enumerate(cases):
        q2, _, _, t2, sl2, ql2 = _fill(Hq, Hkv, dh, vt, T, seqs, 10 + i, kc,
                                       vc, pool)
        q.copy_(q2)
        table.zero_()
        table[:, :t2.shape[1]] = t2
        sl.copy_(sl2)
        ql.copy_(ql2)
        g.replay()
        torch.cuda.synchronize()
        _check(out, q, kc, vc, table, sl, ql, f"replay {i} {seqs}")


def _dh128_gemma():
    return dataclasses.replace(get_config("smoke-gemma"),
                               name="smoke-gemma-dh128", head_dim=128,
                               num_heads=4, num_kv_heads=4)


@pytest.mark.parametrize("name", ["smoke-llama", "smoke-gemma"])
def test_model_verify_matches_cpu(name):
    """prefill() of three prompts' prefixes (20, 0, 16 tokens), then ONE
    verify over 4, 3 and 1 more tokens (T = 4) must give, for every real
    row, the logits of a one-pass fp32 forward at that position, and leave
    KV that decode can use (relative 3e-2, the project's model bound).
    smoke-gemma has head_dim 256, which verify does not serve: its Dh-128
    variant stands in."""
    assert ops.has_hip()
    cfg = get_config(name)
    if cfg.head_dim == 256:
        cfg = _dh128_gemma()
    pre, qn, T = [20, 0, 16], [4, 3, 1], 4
    lens = [p + t for p, t in zip(pre, qn)]
    g = torch.Generator().manual_seed(5)
    prompts = [torch.randint(1, 500, (s,), generator=g).tolist()
               for s in lens]
    m = build_model(cfg, dtype=torch.bfloat16, device=DEV, seed=11)
    fuse_for_inference(m)
    cpu = build_model(cfg, dtype=torch.float32, seed=11)
    cpu.load_state_dict({k: v.float().cpu() for k, v in m.state_dict().items()})
    caches = m.alloc_caches(16, DEV)
    caches_c = cpu.alloc_caches(16, "cpu")
    rows = [[0, 1, 2], [3], [4, 5]]
    dummy = 15
    bt = torch.full((3, 3), dummy, dtype=torch.int32)
    for b, r in enumerate(rows):
        bt[b, :len(r)] = torch.tensor(r, dtype=torch.int32)

    def slots(b, lo, hi):
        return [rows[b][p // BS] * BS + p % BS for p in range(lo, hi)]

    def i32(x, dev):
        return torch.tensor(x, dtype=torch.int32, device=dev)

    def decode(model, caches, dev):
        t = torch.tensor([3, 4, 5], dtype=torch.long, device=dev)
        sl = i32([slots(b, lens[b], lens[b] + 1)[0] for b in range(3)], dev)
        return model.decode(t, i32(lens, dev), caches, sl, bt.to(dev),
                            i32([s + 1 for s in lens], dev))

    with torch.no_grad():
        for b in range(3):
            if pre[b]:
                m.prefill(torch.tensor([prompts[b][:pre[b]]], device=DEV),
                          i32(list(range(pre[b])), DEV), caches,
                          i32(slots(b, 0, pre[b]), DEV))
        toks = [prompts[b][pre[b]:] + [0] * (T - qn[b]) for b in range(3)]
        pos = [list(range(pre[b], lens[b])) + [lens[b] - 1] * (T - qn[b])
               for b in range(3)]
        sl = [slots(b, pre[b], lens[b]) + [dummy * BS] * (T - qn[b])
              for b in range(3)]
        lv = m.verify(torch.tensor(toks, dtype=torch.long, device=DEV),
                      i32(pos, DEV), caches, i32(sl, DEV), bt.to(DEV),
                      i32(lens, DEV), i32(qn, DEV), nsplit=2)
        ld_g = decode(m, caches, DEV)
        full = [cpu(torch.tensor([prompts[b]]))[0] for b in range(3)]
        for b in range(3):
            cpu.prefill(torch.tensor([prompts[b]]),
                        i32(list(range(lens[b])), "cpu"), caches_c,
                        i32(slots(b, 0, lens[b]), "cpu"))
        ld_c = decode(cpu, caches_c, "cpu")
    assert lv.shape == (3 * T, cfg.vocab_size)
    lv = lv.float().cpu().view(3, T, -1)

    def close(what, got, ref):
        rel = (got - ref).abs().max().item() / ref.abs().max().item()
        print(f"{cfg.name} {what}: rel err {rel:.3e}")
        assert rel < 3e-2, (what, got[:8], ref[:8])

    for b in range(3):
        for j in range(qn[b]):
            close(f"verify seq {b} row {j}", lv[b, j], full[b][pre[b] + j])
        close(f"decode seq {b}", ld_g[b].float().cpu(), ld_c[b])


class _Oracle:
    """Proposes the recorded continuation of each request."""

    def __init__(self, by_prompt):
        self.by_prompt = by_prompt

    def propose(self, req, k):
        full = self.by_prompt[tuple(req.prompt_ids)]
        n = len(req.output_ids)
        return full[n:n + k]


def _teacher_forced_ok(cpu, prompt, out):
    """Every emitted token is within 2 x 3e-2 x max|ref| of the fp32 argmax
    logit at its position (the GPU logits may be off by the project's bound
    at the emitted token and at the fp32 argmax)."""
    with torch.no_grad():
        ref = cpu(torch.tensor([prompt + out]))[0]
    for i, t in enumerate(out):
        row = ref[len(prompt) - 1 + i]
        slack = 2 * 3e-2 * row.abs().max().item()
        assert row[t].item() >= row.max().item() - slack, \
            (i, t, row[t].item(), row.max().item(), slack)


def test_engine_speculative_gpu():
    assert ops.has_hip()
    cpu = build_model("smoke-llama", dtype=torch.float32, seed=4)
    pattern = [17, 230, 5, 99, 310, 42, 7, 128]
    prompts = [pattern * 4, [(i * 7 + 3) % 500 + 1 for i in range(21)],
               [3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5]]
    N = 20

    def run(**kw):
        # a fresh, identically seeded model per engine: each engine fuses
        # and registers its own weights
        m = build_model("smoke-llama", dtype=torch.bfloat16, seed=4)
        eng = Engine(m, device=DEV, kv_blocks=128, seed=11, **kw)
        reqs = [eng.submit(p, max_new_tokens=N) for p in prompts]
        for _ in range(200):
            if not eng.has_work():
                break
            eng.step()
        assert not eng.has_work()
        return eng, reqs

    base, ref = run(batch_sampler=True)
    cpu.load_state_dict({k: v.float().cpu()
                         for k, v in base.model.state_dict().items()})
    oracle = _Oracle({tuple(p): r.output_ids for p, r in zip(prompts, ref)})
    for what, kw in (("oracle", dict(drafter=oracle)), ("ngram", {})):
        eng, reqs = run(speculative=4, **kw)
        if what == "ngram":
            assert isinstance(eng.drafter, NgramDrafter)
        print(what, {k: v for k, v in eng.stats.items()
                     if k.startswith("spec") or k in ("steps",
                                                      "decode_tokens")})
        for p, r in zip(prompts, reqs):
            assert r.finished and len(r.output_ids) == N
            _teacher_forced_ok(cpu, p, r.output_ids)
        assert eng.stats["spec_steps"] > 0 and eng.stats["spec_drafted"] > 0
        if what == "oracle":
            assert eng.stats["spec_accepted"] > 0
            assert eng.stats["steps"] < base.stats["steps"]
        assert any(isinstance(k, tuple) and k[1] == "verify"
                   for k in eng._graphed.graphs), "verify graph family unused"
        eng.flush_prefix_cache()
        assert len(eng.allocator.free) == eng.allocator.num_blocks
