"""Prefill from the paged KV cache on CPU: the fp32 reference op, and the
engine's prefill_from_cache / prefill_chunk scheduling (fp32 tiny-llama).

Token comparisons between two engines are only meaningful where fp32
reassociation cannot flip an argmax, so every comparison first checks
that the no-cache forward's top-2 logit gap exceeds 1e-3 at each step.
"""
import pytest
import torch

from runbooks_amd import ops
from runbooks_amd.models import build_model
from runbooks_amd.models.transformer import Transformer
from runbooks_amd.serve import Engine

BS = ops.BLOCK_SIZE


def _fill_cache(k, v, vt, seed):
    """k, v [S, Hkv, Dh] fp32 -> caches filled through a shuffled,
    non-contiguous block table."""
    S, hkv, dh = k.shape
    nb = (S + BS - 1) // BS
    g = torch.Generator().manual_seed(seed)
    table = torch.randperm(2 * nb + 3, generator=g)[:nb].to(torch.int32)
    kc, vc = ops.alloc_kv_cache(2 * nb + 3, hkv, dh, "cpu",
                                dtype=torch.float32, v_transposed=vt)
    pos = torch.arange(S)
    slots = (table[pos // BS].long() * BS + pos % BS).to(torch.int32)
    ops.kv_append_ref(k, v, kc, vc, slots)
    return kc, vc, table


@pytest.mark.parametrize("vt", [False, True])
@pytest.mark.parametrize("P", [0, 16, 48])
def test_paged_prefill_ref_matches_causal_rows(P, vt):
    torch.manual_seed(P + 7 * vt)
    T, hq, hkv, dh = 21, 4, 2, 32          # GQA group of 2
    S = P + T
    q = torch.randn(S, hq, dh)
    k = torch.randn(S, hkv, dh)
    v = torch.randn(S, hkv, dh)
    kc, vc, table = _fill_cache(k, v, vt, seed=P)
    assert ops.attention._is_vt(kc, vc) == vt
    want = ops.attention.causal_attention_ref(q[None], k[None], v[None])[0, P:]
    got = ops.paged_prefill_ref(q[P:], kc, vc, table, P)
    assert got.shape == want.shape
    assert (got - want).abs().max().item() < 1e-5
    # the public op takes the reference path on CPU
    got2 = ops.paged_prefill(q[P:], kc, vc, table, P)
    assert torch.equal(got, got2)


# --- engine ------------------------------------------------------------------

def _model():
    return build_model("tiny-llama", dtype=torch.float32)


def _engine(m, **kw):
    kw.setdefault("kv_blocks", 64)
    return Engine(m, device="cpu", dtype=torch.float32, seed=3, **kw)


def _assert_decisive(m, prompt, output):
    """The no-cache forward picks every token of `output` with a top-2
    logit gap > 1e-3, so engines that differ only in fp32 summation order
    must agree on it."""
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


def test_prefill_from_cache_matches_uncached():
    m = _model()
    sys_prompt = list(range(1, 33))            # 2 full chunks
    prompts = [sys_prompt + [40 + i] for i in range(3)]
    base = _engine(m, prefix_cache=False)
    want = [base.generate(list(p), max_new_tokens=5) for p in prompts]
    for p, w in zip(prompts, want):
        _assert_decisive(m, p, w)

    eng = _engine(m, prefix_cache=True, prefill_from_cache=True)
    reqs = [eng.submit(list(p), max_new_tokens=5) for p in prompts]
    _drain(eng)
    assert [r.output_ids for r in reqs] == want
    assert eng.stats["prefix_hits"] == 2
    assert eng.stats["prefix_skipped_tokens"] == 32 * 2
    # first prompt in full, then one token per hit
    assert eng.stats["prefill_tokens"] == 33 + 1 + 1
    assert eng.stats["prefill_chunks"] == 0
    eng.flush_prefix_cache()
    assert len(eng.allocator.free) == eng.allocator.num_blocks


def test_fully_cached_prompt_still_yields_first_token():
    m = _model()
    prompt = list(range(1, 33))                # S = 32: every chunk can hit
    base = _engine(m, prefix_cache=False)
    want = base.generate(list(prompt), max_new_tokens=4)
    _assert_decisive(m, prompt, want)

    eng = _engine(m, prefix_cache=True, prefill_from_cache=True)
    assert eng.generate(list(prompt), max_new_tokens=4) == want
    assert eng.stats["prefix_skipped_tokens"] == 0
    r = eng.submit(list(prompt), max_new_tokens=4)
    _drain(eng)
    assert r._shared_chunks == 2
    assert r.output_ids == want
    # one token is always computed
    assert eng.stats["prefix_skipped_tokens"] == 31
    assert eng.stats["prefill_tokens"] == 32 + 1
    eng.flush_prefix_cache()
    assert len(eng.allocator.free) == eng.allocator.num_blocks


LONG = [(i * 7 + 3) % 250 + 1 for i in range(50)]


def test_chunked_prefill_interleaves_with_decode():
    m = _model()
    base = _engine(m, prefix_cache=False)
    want_a = base.generate([5, 9, 2], max_new_tokens=12)
    want_b = base.generate(list(LONG), max_new_tokens=4)
    _assert_decisive(m, [5, 9, 2], want_a)
    _assert_decisive(m, LONG, want_b)

    eng = _engine(m, prefix_cache=False, prefill_chunk=16)
    a = eng.submit([5, 9, 2], max_new_tokens=12)
    eng.step()
    assert len(a.output_ids) == 2 and eng.stats["prefill_chunks"] == 0
    b = eng.submit(list(LONG), max_new_tokens=4)
    for i in range(4):                          # 16 + 16 + 16 + 2 tokens
        n0 = len(a.output_ids)
        eng.step()
        assert len(a.output_ids) == n0 + 1, "running request starved"
        if i < 3:
            assert eng.prefilling is b and b not in eng.running
            assert b.computed == 16 * (i + 1) and not b.output_ids
            assert eng.has_work()
    assert eng.prefilling is None and b in eng.running
    assert eng.stats["prefill_chunks"] == 4
    assert eng.stats["prefill_tokens"] == 3 + 50
    _drain(eng)
    assert a.output_ids == want_a
    assert b.output_ids == want_b
    assert len(eng.allocator.free) == eng.allocator.num_blocks


def test_cancel_mid_prefill_releases_blocks():
    eng = _engine(_model(), prefix_cache=False, prefill_chunk=16)
    r = eng.submit(list(LONG), max_new_tokens=4)
    eng.step()
    eng.step()
    assert eng.prefilling is r and r.computed == 32
    assert len(eng.allocator.free) < eng.allocator.num_blocks
    # nothing else is admitted while a prefill is in flight
    other = eng.submit([1, 2, 3], max_new_tokens=2)
    assert eng._admit() is None
    assert eng.cancel(r.request_id)
    assert r.finished and eng.prefilling is None and not r.blocks
    assert len(eng.allocator.free) == eng.allocator.num_blocks
    _drain(eng)
    assert other.finished and len(other.output_ids) == 2
    assert len(eng.allocator.free) == eng.allocator.num_blocks


def test_failure_mid_prefill_releases_blocks(monkeypatch):
    m = _model()
    eng = _engine(m, prefix_cache=False, prefill_chunk=16)
    r = eng.submit(list(LONG), max_new_tokens=4)
    eng.step()
    assert eng.prefilling is r

    def boom(*a, **k):
        raise RuntimeError("chunk failed")
    monkeypatch.setattr(m, "prefill_paged", boom)
    with pytest.raises(RuntimeError, match="chunk failed"):
        eng.step()
    assert r.finished and eng.prefilling is None and not eng.has_work()
    assert len(eng.allocator.free) == eng.allocator.num_blocks


def test_chunk_composes_with_prefix_hit():
    m = _model()
    base = _engine(m, prefix_cache=False)
    want = base.generate(list(LONG), max_new_tokens=4)
    _assert_decisive(m, LONG, want)
    eng = _engine(m, prefix_cache=True, prefill_from_cache=True,
                  prefill_chunk=16)
    eng.generate(LONG[:20] + [7], max_new_tokens=1)   # caches chunk 0
    tok0, ch0 = eng.stats["prefill_tokens"], eng.stats["prefill_chunks"]
    assert eng.generate(list(LONG), max_new_tokens=4) == want
    # first chunk starts at ctx_len = 16: 16 + 16 + 2 tokens
    assert eng.stats["prefix_skipped_tokens"] == 16
    assert eng.stats["prefill_tokens"] - tok0 == 34
    assert eng.stats["prefill_chunks"] - ch0 == 3


def test_prefill_chunk_must_be_block_multiple():
    with pytest.raises(ValueError):
        _engine(_model(), prefill_chunk=24)


def test_preempted_request_readmits_from_cache():
    """Small pool, as in test_kv_preemption_under_pressure: a preempted
    request's history is still in the prefix cache, so its re-prefill
    skips it, and the output is what an unpressured engine produces."""
    m = _model()
    # constant prompts whose greedy continuation is decisive (checked below)
    prompts = [[t] * 30 for t in (19, 30, 32)]
    big = _engine(m, prefix_cache=False)
    want = [big.generate(list(p), max_new_tokens=24) for p in prompts]
    for p, w in zip(prompts, want):
        _assert_decisive(m, p, w)

    # 7 usable blocks: two 54-token sequences (4 blocks each) overflow it
    eng = _engine(m, kv_blocks=8, prefix_cache=True, prefill_from_cache=True)
    reqs = [eng.submit(list(p), max_new_tokens=24) for p in prompts]
    _drain(eng)
    assert eng.stats["preemptions"] > 0
    assert eng.stats["prefix_skipped_tokens"] > 0
    for r, w in zip(reqs, want):
        assert r.finished
        assert r.prompt_ids[30:] + r.output_ids == w
    eng.flush_prefix_cache()
    assert len(eng.allocator.free) == eng.allocator.num_blocks


def test_defaults_never_call_prefill_paged(monkeypatch):
    monkeypatch.delenv("RB_PREFILL_FROM_CACHE", raising=False)
    monkeypatch.delenv("RB_PREFILL_CHUNK", raising=False)

    def boom(*a, **k):
        raise AssertionError("prefill_paged called with both knobs unset")
    monkeypatch.setattr(Transformer, "prefill_paged", boom)
    eng = _engine(_model(), prefix_cache=True)
    assert not eng.prefill_from_cache and eng.prefill_chunk == 0
    sys_prompt = list(range(1, 33))
    for i in range(3):
        assert len(eng.generate(sys_prompt + [40 + i], max_new_tokens=3)) == 3
    assert len(eng.generate(list(LONG), max_new_tokens=2)) == 2
    assert eng.stats["prefix_hits"] == 2
    assert eng.stats["prefix_skipped_tokens"] == 0
    assert eng.stats["prefill_tokens"] == 33 * 3 + 50


def test_server_main_reads_prefill_params(tmp_path, monkeypatch):
    """PARAM_PREFILL_FROM_CACHE / PARAM_PREFILL_CHUNK reach the engine."""
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
    monkeypatch.setenv("PARAM_PREFILL_FROM_CACHE", "true")
    monkeypatch.setenv("PARAM_PREFILL_CHUNK", "32")
    got = {}
    monkeypatch.setattr(http_mod, "serve_forever",
                        lambda engine, *a, **k: got.update(engine=engine))
    assert server_main.main() == 0
    assert got["engine"].prefill_from_cache is True
    assert got["engine"].prefill_chunk == 32
    assert len(got["engine"].generate(list(LONG), max_new_tokens=2)) == 2
    assert got["engine"].stats["prefill_chunks"] == 2
