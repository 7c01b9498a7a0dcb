"""Batched (packed, "varlen") paged prefill on CPU: the fp32 reference op
and its host checks, and the engine's prefill_batch scheduling (fp32
tiny-llama).

As in test_paged_prefill_cpu.py, token comparisons between two engines
first check that the no-cache forward's top-2 logit gap exceeds 1e-3 at
each step, so fp32 reassociation (another M in the linears) cannot flip
an argmax.
"""
import pytest
import torch

from runbooks_amd import ops
from runbooks_amd.models import build_model
from runbooks_amd.models.transformer import Transformer
from runbooks_amd.serve import Engine

BS = ops.BLOCK_SIZE


# --- reference op -------------------------------------------------------------

@pytest.mark.parametrize("vt", [False, True])
def test_batch_ref_equals_per_sequence_ref(vt):
    torch.manual_seed(3 + vt)
    hq, hkv, dh = 4, 2, 32
    seqs = [(0, 21), (48, 5), (16, 1), (20, 40)]       # (ctx, T)
    pool = 32
    kc, vc = ops.alloc_kv_cache(pool, hkv, dh, "cpu", dtype=torch.float32,
                                v_transposed=vt)
    assert ops.attention._is_vt(kc, vc) == vt
    g = torch.Generator().manual_seed(9)
    perm = torch.randperm(pool, generator=g).tolist()
    maxb = max((c + t + BS - 1) // BS for c, t in seqs) + 2
    bt = torch.full((len(seqs), maxb), perm.pop(), dtype=torch.int32)
    qs, ks, vs = [], [], []
    for b, (ctx, T) in enumerate(seqs):
        S = ctx + T
        nb = (S + BS - 1) // BS
        blocks = [perm.pop() for _ in range(nb)]
        k = torch.randn(S, hkv, dh)
        v = torch.randn(S, hkv, dh)
        pos = torch.arange(S)
        if b == 2:
            # a prefix hit: sequence 2's first block IS sequence 1's first
            # block, already written; only its own token is appended
            blocks[0] = int(bt[1, 0])
            k[:BS], v[:BS] = ks[1][:BS], vs[1][:BS]
            pos = pos[BS:]
        bt[b, :nb] = torch.tensor(blocks, dtype=torch.int32)
        slots = (bt[b][pos // BS].long() * BS + pos % BS).to(torch.int32)
        ops.kv_append_ref(k[pos], v[pos], kc, vc, slots)
        qs.append(torch.randn(T, hq, dh))
        ks.append(k)
        vs.append(v)
    q = torch.cat(qs)
    plan = ops.paged_prefill_plan([t for _, t in seqs], [c for c, _ in seqs],
                                  "cpu")
    assert plan.total == q.shape[0] and plan.dev is None
    got = ops.paged_prefill_batch_ref(q, kc, vc, bt, plan)
    lo = 0
    for b, (ctx, T) in enumerate(seqs):
        want = ops.paged_prefill_ref(qs[b], kc, vc, bt[b], ctx)
        assert torch.equal(got[lo:lo + T], want), f"sequence {b}"
        lo += T
    # the public op takes the reference path on CPU
    assert torch.equal(ops.paged_prefill_batch(q, kc, vc, bt, plan), got)


def test_plan_layout_and_checks():
    plan = ops.paged_prefill_plan([3, 300, 1], [0, 5, 16], "cpu")
    # [cu_q | ctx | tile_seq | tile_row0]; the 300-row sequence has 2 tiles
    assert plan.cpu.tolist() == [0, 3, 303, 304, 0, 5, 16,
                                 0, 1, 1, 2, 0, 0, 256, 0]
    assert plan.ntiles == 4 and plan.num_seqs == 3
    assert plan.last_rows().tolist() == [2, 302, 303]
    assert plan.max_blocks() == (5 + 300 + 15) // 16
    for q_lens, ctx in (([4, 0], [0, 0]), ([4], [-1]), ([], []),
                        ([4, 4], [0]), ([1], [(1 << 30) - 1])):
        with pytest.raises(ValueError):
            ops.paged_prefill_plan(q_lens, ctx, "cpu")
    kc, vc = ops.alloc_kv_cache(4, 1, 32, "cpu", dtype=torch.float32)
    plan = ops.paged_prefill_plan([4, 20], [0, 16], "cpu")
    q = torch.zeros(24, 2, 32)
    bt = torch.zeros(2, 3, dtype=torch.int32)
    ops.paged_prefill_batch(q, kc, vc, bt, plan)
    with pytest.raises(ValueError):           # q rows != sum T_b
        ops.paged_prefill_batch(q[:23], kc, vc, bt, plan)
    with pytest.raises(ValueError):           # table too narrow
        ops.paged_prefill_batch(q, kc, vc, bt[:, :2], plan)
    with pytest.raises(ValueError):           # B mismatch
        ops.paged_prefill_batch(q, kc, vc, bt[:1], plan)


# --- engine ------------------------------------------------------------------

def _model():
    return build_model("tiny-llama", dtype=torch.float32)


def _engine(m, **kw):
    kw.setdefault("kv_blocks", 64)
    return Engine(m, device="cpu", dtype=torch.float32, seed=3, **kw)


def _assert_decisive(m, prompt, output):
    seq = list(prompt) + list(output)
    with torch.no_grad():
        logits = m(torch.tensor([seq]))[0]
    for i, tok in enumerate(output):
        row = logits[len(prompt) - 1 + i]
        top = row.topk(2)
        assert int(top.indices[0]) == tok
        assert float(top.values[0] - top.values[1]) > 1e-3, \
            "baseline argmax too close to call; pick other prompts"


def _drain(eng):
    for _ in range(500):
        if not eng.has_work():
            return
        eng.step()
    raise AssertionError("scheduler wedged")


def _count_prefills(monkeypatch, m):
    """Wrap every model.*prefill* entry point of instance m with a
    counter."""
    calls = {"n": 0, "batch": 0}
    for name in ("prefill", "prefill_paged", "prefill_paged_batch"):
        orig = getattr(m, name)

        def wrapped(*a, _orig=orig, _name=name, **k):
            calls["n"] += 1
            calls["batch"] += _name == "prefill_paged_batch"
            return _orig(*a, **k)
        monkeypatch.setattr(m, name, wrapped)
    return calls


SYS = list(range(1, 33))                        # two full 16-token chunks
LONG = [(i * 7 + 3) % 250 + 1 for i in range(50)]


def test_prefill_batch_matches_unbatched(monkeypatch):
    m = _model()
    prompts = [SYS + [40], SYS + [41], [5, 9, 2], SYS + [42], list(LONG),
               [19] * 12]
    n_new = 4
    base = _engine(m, prefix_cache=False)
    want = [base.generate(list(p), max_new_tokens=n_new) for p in prompts]
    for p, w in zip(prompts, want):
        _assert_decisive(m, p, w)

    calls = _count_prefills(monkeypatch, m)
    got, n_calls, stats = {}, {}, {}
    for pb in (0, 4):
        calls["n"] = calls["batch"] = 0
        eng = _engine(m, prefix_cache=True, prefill_from_cache=True,
                      prefill_chunk=16, prefill_batch=pb)
        eng.max_prefills_per_step = 4
        reqs = [eng.submit(list(p), max_new_tokens=n_new) for p in prompts]
        _drain(eng)
        got[pb] = [r.output_ids for r in reqs]
        n_calls[pb] = dict(calls)
        stats[pb] = dict(eng.stats)
        eng.flush_prefix_cache()
        assert len(eng.allocator.free) == eng.allocator.num_blocks
    assert got[0] == want
    assert got[4] == want
    assert n_calls[0]["batch"] == 0 and stats[0]["prefill_batches"] == 0
    assert n_calls[4]["batch"] >= 1
    assert n_calls[4]["n"] < n_calls[0]["n"], n_calls
    assert stats[4]["prefill_batches"] == n_calls[4]["batch"]
    assert stats[4]["prefill_batched_requests"] >= 2
    # the counters keep their meaning: same prompts, same hits
    for key in ("prefills", "prefill_tokens", "prefix_skipped_tokens"):
        assert stats[4][key] == stats[0][key], key
    # the 33- and 50-token prompts exceed prefill_chunk: chunked, alone
    assert stats[4]["prefill_chunks"] == stats[0]["prefill_chunks"] == 3 + 4


def test_in_batch_prefix_rule_defers_the_hit():
    m = _model()
    head = list(range(1, 17))                   # one full shared block
    eng = _engine(m, prefix_cache=True, prefill_from_cache=True,
                  prefill_batch=4)
    a = eng.submit(head + [40, 41], max_new_tokens=3)
    b = eng.submit(head + [50], max_new_tokens=3)
    eng.step()
    # b would hit on the block a publishes in this very step: it waits
    assert eng.waiting == [b] and a.output_ids
    assert eng.stats["prefill_batches"] == 0 and eng.stats["prefills"] == 1
    eng.step()
    assert b.output_ids and not eng.waiting
    assert eng.stats["prefix_hits"] == 1
    assert eng.stats["prefix_skipped_tokens"] == 16
    _drain(eng)
    eng.flush_prefix_cache()
    assert len(eng.allocator.free) == eng.allocator.num_blocks


def test_prefill_chunk_is_the_batch_token_budget():
    m = _model()
    eng = _engine(m, prefix_cache=False, prefill_chunk=32, prefill_batch=4)
    reqs = [eng.submit([(7 * i + j) % 200 + 1 for j in range(20)],
                       max_new_tokens=2) for i in range(3)]
    for left in (2, 1, 0):                      # 20 + 20 > 32: one per step
        eng.step()
        assert len(eng.waiting) == left
    _drain(eng)
    assert all(r.finished and len(r.output_ids) == 2 for r in reqs)
    assert eng.stats["prefill_batches"] == 0 and eng.stats["prefills"] == 3

    eng = _engine(m, prefix_cache=False, prefill_chunk=32, prefill_batch=4)
    reqs = [eng.submit([(7 * i + j) % 200 + 1 for j in range(10)],
                       max_new_tokens=2) for i in range(3)]
    eng.step()
    assert not eng.waiting
    assert eng.stats["prefill_batches"] == 1
    assert eng.stats["prefill_batched_requests"] == 3
    assert eng.stats["prefill_tokens"] == 30 and eng.stats["prefills"] == 3
    _drain(eng)
    assert all(r.finished and len(r.output_ids) == 2 for r in reqs)
    assert len(eng.allocator.free) == eng.allocator.num_blocks


def test_prefill_batch_respects_max_batch():
    eng = _engine(_model(), prefix_cache=False, prefill_batch=8, max_batch=3)
    reqs = [eng.submit([3 + i, 4, 5], max_new_tokens=8) for i in range(5)]
    eng.step()
    assert len(eng.running) == 3 and len(eng.waiting) == 2
    assert eng.stats["prefill_batched_requests"] == 3
    _drain(eng)
    assert all(r.finished and len(r.output_ids) == 8 for r in reqs)


def test_failure_in_batched_forward_releases_every_member(monkeypatch):
    m = _model()
    eng = _engine(m, prefix_cache=True, prefill_from_cache=True,
                  prefill_batch=4)
    eng.generate(SYS + [7], max_new_tokens=1)   # publishes two blocks
    held = eng.allocator.num_blocks - len(eng.allocator.free)
    assert held == 2
    reqs = [eng.submit(SYS + [40 + i], max_new_tokens=3) for i in range(2)]
    reqs.append(eng.submit([9, 8, 7, 6], max_new_tokens=3))

    def boom(*a, **k):
        raise RuntimeError("batched forward failed")
    monkeypatch.setattr(m, "prefill_paged_batch", boom)
    with pytest.raises(RuntimeError, match="batched forward failed"):
        eng.step()
    assert all(r.finished and not r.blocks for r in reqs)
    assert not eng.has_work()
    # only the prefix cache's own two references remain
    assert eng.allocator.num_blocks - len(eng.allocator.free) == held
    eng.flush_prefix_cache()
    assert len(eng.allocator.free) == eng.allocator.num_blocks


def test_defaults_never_call_prefill_paged_batch(monkeypatch):
    monkeypatch.delenv("RB_PREFILL_BATCH", raising=False)

    def boom(*a, **k):
        raise AssertionError("prefill_paged_batch called with the knob unset")
    monkeypatch.setattr(Transformer, "prefill_paged_batch", boom)
    eng = _engine(_model(), prefix_cache=True, prefill_from_cache=True)
    assert eng.prefill_batch == 0
    eng.max_prefills_per_step = 4
    reqs = [eng.submit(SYS + [40 + i], max_new_tokens=3) for i in range(3)]
    reqs.append(eng.submit([5, 9, 2], max_new_tokens=3))
    eng.step()
    # today's cadence: max_prefills_per_step admissions, one forward each
    assert not eng.waiting and eng.stats["prefills"] == 4
    _drain(eng)
    assert all(len(r.output_ids) == 3 for r in reqs)
    assert eng.stats["prefill_batches"] == 0
    assert eng.stats["prefill_batched_requests"] == 0


def test_prefill_batch_env_and_validation(monkeypatch):
    monkeypatch.setenv("RB_PREFILL_BATCH", "3")
    assert _engine(_model()).prefill_batch == 3
    assert _engine(_model(), prefill_batch=0).prefill_batch == 0
    with pytest.raises(ValueError):
        _engine(_model(), prefill_batch=-1)


def test_server_main_reads_prefill_batch(tmp_path, monkeypatch):
    """PARAM_PREFILL_BATCH reaches the engine."""
    import json

    import runbooks_amd.serve.http as http_mod
    from runbooks_amd.workloads import server_main
    model_dir = tmp_path / "model"
    model_dir.mkdir()
    (model_dir / "config.json").write_text(
        json.dumps({"runbooks_amd_config": "tiny-llama"}))
    monkeypatch.setenv("MODEL_DIR", str(model_dir))
    monkeypatch.delenv("TP", raising=False)
    # keep the tiny model on the CPU wherever the test runs
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setenv("PARAM_PREFILL_BATCH", "4")
    got = {}
    monkeypatch.setattr(http_mod, "serve_forever",
                        lambda engine, *a, **k: got.update(engine=engine))
    assert server_main.main() == 0
    eng = got["engine"]
    assert eng.prefill_batch == 4
    reqs = [eng.submit([3 + i, 4, 5, 6], max_new_tokens=2) for i in range(3)]
    _drain(eng)
    assert all(len(r.output_ids) == 2 for r in reqs)
    assert eng.stats["prefill_batches"] == 1
    assert eng.stats["prefill_batched_requests"] == 3
