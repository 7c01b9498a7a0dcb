"""Speculative decoding on the CPU reference path (fp32, smoke-llama):
ops.paged_verify_ref, the n-gram drafter, and the engine's speculative step
against the non-speculative batched-sampler engine, token for token."""
import pytest
import torch

from runbooks_amd import ops
from runbooks_amd.models import build_model, get_config
from runbooks_amd.serve import Engine, NgramDrafter, Request

BS = ops.BLOCK_SIZE
NAN = float("nan")
PROMPTS = [[17, 230, 5, 99, 310, 42, 7, 128] * 3,
           [(i * 7 + 3) % 500 + 1 for i in range(21)],
           [3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5]]
N_NEW = 24
MODEL_SEED = 9


# -- paged_verify_ref ---------------------------------------------------------
@pytest.mark.parametrize("vt", [False, True])
def test_paged_verify_ref(vt):
    torch.manual_seed(0)
    Hq, Hkv, dh, T = 4, 2, 32, 4
    seqs = [(20, 4), (5, 2), (9, 0), (33, 1)]      # (seq_len, q_len)
    kc, vc = ops.alloc_kv_cache(12, Hkv, dh, "cpu", dtype=torch.float32,
                                v_transposed=vt)
    spare = 11
    kc[spare] = NAN
    vc[spare] = NAN
    table = torch.full((4, 4), spare, dtype=torch.int32)
    nxt = 0
    for b, (S, n) in enumerate(seqs):
        if n == 0:
            continue                                # row b: all NaN block
        nb = (S + BS - 1) // BS
        table[b, :nb] = torch.arange(nxt, nxt + nb, dtype=torch.int32)
        nxt += nb
        pos = torch.arange(S)
        slots = (table[b][pos // BS].long() * BS + pos % BS).to(torch.int32)
        ops.kv_append(torch.randn(S, Hkv, dh), torch.randn(S, Hkv, dh), kc,
                      vc, slots)
    q = torch.randn(4, T, Hq, dh)
    sl = torch.tensor([s for s, _ in seqs], dtype=torch.int32)
    ql = torch.tensor([n for _, n in seqs], dtype=torch.int32)
    out = ops.paged_verify(q, kc, vc, table, sl, ql)     # CPU path == ref
    assert torch.equal(out, ops.paged_verify_ref(q, kc, vc, table, sl, ql))
    assert not torch.isnan(out).any()
    for b, (S, n) in enumerate(seqs):
        assert (out[b, n:] == 0).all()
        if n:
            ref = ops.paged_prefill_ref(q[b, :n], kc, vc, table[b], S - n)
            assert torch.equal(out[b, :n], ref)
    with pytest.raises(ValueError):
        ops.paged_verify_ref(q.repeat(1, 3, 1, 1), kc, vc, table, sl, ql)
    with pytest.raises(TypeError):
        ops.paged_verify_ref(q, kc, vc, table, sl, ql.long())
    with pytest.raises(ValueError):
        ops.paged_verify_ref(q, kc, vc, table[:2], sl, ql)


# -- NgramDrafter -------------------------------------------------------------
def _req(prompt, out=(), rid=0):
    r = Request(rid, list(prompt))
    r.output_ids = list(out)
    return r


def test_ngram_drafter_matches():
    d = NgramDrafter(3)
    # longest suffix wins: "1 2 3" (-> 7) over the later "2 3" (-> 9)
    assert d.propose(_req([1, 2, 3, 7, 8, 5, 2, 3, 9, 1, 2, 3]), 2) == [7, 8]
    # most recent match of the same length: "2 3" -> 9, not 4
    assert d.propose(_req([2, 3, 4, 2, 3, 9, 6, 2, 3], rid=1), 3) == [9, 6, 2]
    # falls back to shorter suffixes, down to one token
    assert d.propose(_req([5, 6, 7, 1, 6], rid=2), 4) == [7, 1, 6]
    # no match -> nothing; k bounds the draft; k = 0 -> nothing
    assert d.propose(_req([1, 2, 3, 4], rid=3), 4) == []
    # (the most recent match of a periodic text sits near its end, so the
    # draft may be shorter than k)
    assert d.propose(_req([1, 2] * 10, rid=4), 1) == [1]
    assert len(d.propose(_req([1, 2, 3] * 6, rid=5), 3)) == 3
    assert len(d.propose(_req([1, 2] * 10, rid=6), 7)) <= 7
    assert d.propose(_req([1, 2] * 10, rid=4), 0) == []
    with pytest.raises(ValueError):
        NgramDrafter(0)


def test_ngram_drafter_incremental_equals_rescan():
    g = torch.Generator().manual_seed(1)
    text = torch.randint(0, 6, (120,), generator=g).tolist()
    inc = NgramDrafter(3)
    r = _req(text[:10])
    for i in range(10, len(text)):
        fresh = NgramDrafter(3).propose(_req(text[:i], rid=9), 5)
        r.output_ids = text[10:i]
        assert inc.propose(r, 5) == fresh, i
    # a rewritten history (preemption folds output into the prompt, a
    # recycled id) starts over instead of trusting stale state
    assert inc.propose(_req([4, 4, 4, 4]), 2) == [4]
    inc.forget(0)
    assert 0 not in inc._state


# -- engine -------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    # seed 9: the greedy reference run's smallest top-1/top-2 margin is
    # 2e-3 (test_reference_run_is_well_conditioned)
    return build_model("smoke-llama", dtype=torch.float32, seed=MODEL_SEED)


def _engine(model, **kw):
    kw.setdefault("kv_blocks", 64)
    return Engine(model, device="cpu", dtype=torch.float32, seed=5, **kw)


def _run(eng, prompts=PROMPTS, n=N_NEW, **sub):
    reqs = [eng.submit(p, max_new_tokens=n, **sub) for p in prompts]
    for _ in range(400):
        if not eng.has_work():
            break
        eng.step()
    assert not eng.has_work()
    return reqs


class Oracle:
    """Proposes the recorded continuation; ``wrong_after`` = j makes every
    proposal right for its first j tokens and wrong from there on."""

    def __init__(self, ref, wrong_after=None, vocab=512):
        self.ref = {tuple(p): o for p, o in ref}
        self.wrong_after = wrong_after
        self.vocab = vocab

    def propose(self, req, k):
        n = len(req.output_ids)
        d = list(self.ref[tuple(req.prompt_ids)][n:n + k])
        if self.wrong_after is not None:
            d = [t if j < self.wrong_after else (t + 1) % self.vocab
                 for j, t in enumerate(d)]
        return d


def _reference(model, **sub):
    """Non-speculative batched-sampler run: tokens, steps, and the top-1 to
    top-2 logit margin of every sampled row."""
    eng = _engine(model, batch_sampler=True)
    margins = []
    orig = eng._sample_batched

    def spy(logits, reqs, seed_pos=None):
        top = logits.float().topk(2, dim=-1).values
        margins.extend((top[:, 0] - top[:, 1]).tolist())
        return orig(logits, reqs, seed_pos)

    eng._sample_batched = spy
    reqs = _run(eng, **sub)
    return [r.output_ids for r in reqs], eng.stats["steps"], margins


SAMPLING = [dict(), dict(temperature=0.8, seed=7, top_k=20)]


@pytest.fixture(scope="module", params=[0, 1], ids=["greedy", "seeded"])
def recorded(request, model):
    sub = SAMPLING[request.param]
    toks, steps, margins = _reference(model, **sub)
    return sub, toks, steps, margins


def test_reference_run_is_well_conditioned(recorded):
    """A condition on the greedy reference run: no near-tie that fp32
    summation order in a batched forward could flip (a seeded draw is not
    decided by the top-1/top-2 margin, so it is measured on greedy only)."""
    sub, toks, _, margins = recorded
    assert all(len(t) == N_NEW for t in toks)
    assert len(margins) == 3 * N_NEW
    if not sub:
        assert min(margins) > 1e-3, min(margins)


def test_oracle_drafter_all_accepted(recorded, model):
    sub, toks, steps, _ = recorded
    eng = _engine(model, speculative=4,
                  drafter=Oracle(zip(PROMPTS, toks)))
    reqs = _run(eng, **sub)
    assert [r.output_ids for r in reqs] == toks
    assert eng.stats["spec_accepted"] == eng.stats["spec_drafted"] > 0
    assert eng.stats["steps"] < steps
    assert eng.stats["decode_tokens"] == sum(len(t) - 1 for t in toks)
    eng.flush_prefix_cache()
    assert len(eng.allocator.free) == eng.allocator.num_blocks


def test_always_wrong_drafter(recorded, model):
    sub, toks, _, _ = recorded
    eng = _engine(model, speculative=4,
                  drafter=Oracle(zip(PROMPTS, toks), wrong_after=0))
    reqs = _run(eng, **sub)
    assert [r.output_ids for r in reqs] == toks
    assert eng.stats["spec_accepted"] == 0 < eng.stats["spec_drafted"]


def test_partly_right_drafter(recorded, model):
    sub, toks, _, _ = recorded
    eng = _engine(model, speculative=4,
                  drafter=Oracle(zip(PROMPTS, toks), wrong_after=2))
    reqs = _run(eng, **sub)
    assert [r.output_ids for r in reqs] == toks
    assert 0 < eng.stats["spec_accepted"] < eng.stats["spec_drafted"]


def test_builtin_ngram_drafter(recorded, model):
    sub, toks, _, _ = recorded
    eng = _engine(model, speculative=4, spec_ngram=2)
    assert isinstance(eng.drafter, NgramDrafter) and eng.drafter.n == 2
    reqs = _run(eng, **sub)
    assert [r.output_ids for r in reqs] == toks
    assert eng.drafter._state == {}          # forgotten with the requests


# -- trimming -----------------------------------------------------------------
@pytest.fixture(scope="module")
def greedy(model):
    toks, steps, _ = _reference(model)
    return toks, steps


def test_max_new_tokens_mid_acceptance(greedy, model):
    toks, _ = greedy
    for n in (2, 3, 7):
        eng = _engine(model, speculative=4, drafter=Oracle(zip(PROMPTS, toks)))
        reqs = _run(eng, n=n)
        assert [r.output_ids for r in reqs] == [t[:n] for t in toks]


def _runs(model, toks, i, **sub):
    """One request (prompt i) on a speculative engine with the oracle
    drafter: its output and the [lo, hi) output range each step emitted."""
    eng = _engine(model, speculative=4, drafter=Oracle(zip(PROMPTS, toks)))
    r = eng.submit(PROMPTS[i], max_new_tokens=N_NEW, **sub)
    spans = []
    while eng.has_work():
        lo = len(r.output_ids)
        eng.step()
        spans.append((lo, len(r.output_ids)))
    return r.output_ids, spans, eng


@pytest.mark.parametrize("late", [False, True], ids=["first_run", "later_run"])
def test_stop_id_inside_accepted_run(greedy, model, late):
    """A stop id whose first occurrence lies strictly inside a multi-token
    accepted run (not its last token) ends the output there: the tokens the
    same step would have emitted after it are dropped. Checked for the
    first speculative step and for a later one."""
    toks, _ = greedy
    found = None
    for i in range(len(PROMPTS)):
        out, spans, _ = _runs(model, toks, i)
        assert out == toks[i]
        multi = [(lo, hi) for lo, hi in spans if hi - lo >= 3]
        for lo, hi in (multi[1:] if late else multi[:1]):
            # not the run's last token, and not its first (in the first
            # step that one comes from the prefill)
            for j in range(lo + 1, hi - 1):
                if out[j] not in out[:j]:
                    found = (i, j, lo, hi)
                    break
            if found:
                break
        if found:
            break
    assert found, "no stop candidate inside an accepted run: pick other seeds"
    i, j, lo, hi = found
    out, spans, eng = _runs(model, toks, i, stop_token_ids=(toks[i][j],))
    assert out == toks[i][:j + 1]
    assert spans[-1] == (lo, j + 1) and j + 1 < hi   # the step was cut short
    assert eng.stats["spec_drafted"] > 0
    print(f"stop id {toks[i][j]} at output {j} of prompt {i}: the step's "
          f"run [{lo}, {hi}) ended at {j + 1}")
    assert len(eng.allocator.free) + len(eng._pc) == eng.allocator.num_blocks


def test_draft_token_ids_are_range_checked(greedy, model):
    """A drafter is user code: ids outside the vocabulary never reach the
    embedding; the draft ends before the first one."""
    toks, _ = greedy

    class Rogue(Oracle):
        def propose(self, req, k):
            d = super().propose(req, k)
            return d[:2] + [512 if len(req.output_ids) % 2 else -1] + d[2:]

    eng = _engine(model, speculative=4, drafter=Rogue(zip(PROMPTS, toks)))
    seen = []
    orig = eng.model.verify

    def spy(tokens, *a, **kw):
        seen.append(tokens.clone())
        return orig(tokens, *a, **kw)

    eng.model.verify = spy
    try:
        reqs = _run(eng)
    finally:
        del eng.model.verify
    assert [r.output_ids for r in reqs] == toks
    assert seen and all(int(t.min()) >= 0 and int(t.max()) < 512
                        for t in seen)
    assert eng.stats["spec_accepted"] == eng.stats["spec_drafted"] > 0


def test_cancel_forgets_drafter_state(model):
    """A request cancelled while it waits (for instance after a
    preemption) leaves no drafter state behind."""
    eng = _engine(model, speculative=4)
    r = eng.submit(PROMPTS[0], max_new_tokens=8)
    eng.step()
    eng.step()
    assert r.request_id in eng.drafter._state
    eng._preempt(r)
    assert r in eng.waiting and eng.cancel(r.request_id)
    assert eng.drafter._state == {} and eng._tok_counts == {}


def test_pool_limits_drafts_without_preemption(greedy, model):
    """Five blocks: B (11 tokens, 2 blocks = positions 0..31) drafts 7 a
    step; A (21 tokens, 3 blocks) arrives one step later, drafts nothing
    and holds the rest of the pool until it finishes at the end of step 3.
    In step 3 B is at length 28 with 6 drafts allowed by max_new_tokens,
    which would reach position 33 in a third block: none is free, so 4 are
    run (up to position 31). Nothing is evicted or preempted; the block A
    frees serves B's next step."""
    toks, _ = greedy
    orc = Oracle(zip(PROMPTS, toks))

    class OnlyB:
        def propose(self, req, k):
            return orc.propose(req, k) if req.prompt_ids == PROMPTS[2] else []

    eng = _engine(model, speculative=7, kv_blocks=6, prefix_cache=False,
                  drafter=OnlyB())
    b = eng.submit(PROMPTS[2], max_new_tokens=N_NEW)
    a = eng.submit(PROMPTS[1], max_new_tokens=3)
    drafted, free = [], []
    while eng.has_work():
        before = eng.stats["spec_drafted"]
        eng.step()
        drafted.append(eng.stats["spec_drafted"] - before)
        free.append(len(eng.allocator.free))
    assert b.output_ids == toks[2] and a.output_ids == toks[1][:3]
    assert drafted == [7, 7, 4, 1], (drafted, free)
    assert eng.stats["preemptions"] == 0
    assert eng.stats["spec_accepted"] == eng.stats["spec_drafted"]
    assert len(eng.allocator.free) == eng.allocator.num_blocks


def test_penalty_and_logprob_rows_get_no_drafts(greedy, model):
    toks, _ = greedy

    class Counting(Oracle):
        asked = []

        def propose(self, req, k):
            self.asked.append(req.request_id)
            return [1] * k if tuple(req.prompt_ids) not in self.ref \
                else super().propose(req, k)

    eng = _engine(model, speculative=4, drafter=Counting(zip(PROMPTS, toks)))
    plain = eng.submit(PROMPTS[0], max_new_tokens=12)
    pen = eng.submit([9, 8, 7, 9, 8, 7, 9, 8], max_new_tokens=12,
                     repetition_penalty=1.3)
    lp = eng.submit([4, 4, 4, 4, 4, 4], max_new_tokens=12, logprobs=2)
    while eng.has_work():
        eng.step()
    assert plain.output_ids == toks[0][:12]
    assert set(Counting.asked) == {plain.request_id}
    assert eng.stats["spec_accepted"] > 0
    assert len(lp.logprob_data) == 12 and len(pen.output_ids) == 12
    # the same two requests on a non-speculative engine
    ref = _engine(model, batch_sampler=True)
    ref.submit(PROMPTS[0], max_new_tokens=12)
    pen2 = ref.submit([9, 8, 7, 9, 8, 7, 9, 8], max_new_tokens=12,
                      repetition_penalty=1.3)
    lp2 = ref.submit([4, 4, 4, 4, 4, 4], max_new_tokens=12, logprobs=2)
    while ref.has_work():
        ref.step()
    assert pen.output_ids == pen2.output_ids
    assert lp.output_ids == lp2.output_ids


def test_adapter_row_sends_the_step_down_the_normal_path(greedy, model):
    toks, _ = greedy
    m = build_model("smoke-llama", dtype=torch.float32, seed=MODEL_SEED)
    eng = Engine(m, device="cpu", dtype=torch.float32, seed=5, kv_blocks=64,
                 max_loras=1, lora_rank=16, speculative=4,
                 drafter=Oracle(zip(PROMPTS, toks)))
    state, alpha = _small_adapter(16), 8.0
    eng.load_adapter_state("a", state, alpha, 16)
    # the adapter row is admitted first and outlives the other
    r1 = eng.submit(PROMPTS[1], max_new_tokens=12, adapter="a")
    r0 = eng.submit(PROMPTS[0], max_new_tokens=6)
    while eng.has_work():
        eng.step()
    assert eng.stats["spec_steps"] == 0 and eng.stats["spec_drafted"] == 0
    assert eng.stats["lora_decode_steps"] > 0
    assert len(r0.output_ids) == 6 and len(r1.output_ids) == 12
    assert r0.output_ids == toks[0][:6]


def _small_adapter(r):
    """State dict of a random rank-r adapter in the trainer's layout."""
    from runbooks_amd.train.lora import apply_lora, lora_state_dict
    ref = build_model("smoke-llama", dtype=torch.float32, seed=3)
    apply_lora(ref, r=r, alpha=8)
    g = torch.Generator().manual_seed(0)
    return {k: torch.randn(v.shape, generator=g) * 0.05
            for k, v in lora_state_dict(ref).items()}


# -- knobs --------------------------------------------------------------------
def test_knob_parsing(model, monkeypatch, capsys):
    with pytest.raises(ValueError):
        _engine(model, speculative=8)
    with pytest.raises(ValueError):
        _engine(model, speculative=-1)
    off = _engine(model)
    assert off.speculative == 0 and off.drafter is None
    assert "spec_steps" not in off.stats and off.batch_sampler is False
    monkeypatch.setenv("RB_SPECULATIVE", "3")
    monkeypatch.setenv("RB_SPEC_NGRAM", "5")
    on = _engine(model)
    assert on.speculative == 3 and on.drafter.n == 5 and on.batch_sampler
    assert _engine(model, speculative=0).drafter is None
    monkeypatch.delenv("RB_SPECULATIVE")
    # ignored: fp8 KV cache, sliding window, head_dim 256
    capsys.readouterr()
    e = _engine(model, speculative=4, kv_fp8=True)
    assert e.speculative == 0 and e.drafter is None
    assert "speculative ignored" in capsys.readouterr().out
    import dataclasses
    for cfg in (dataclasses.replace(get_config("smoke-llama"), name="sw",
                                    sliding_window=64),
                dataclasses.replace(get_config("smoke-gemma"), name="g256",
                                    num_layers=1)):
        e = Engine(build_model(cfg, dtype=torch.float32), device="cpu",
                   dtype=torch.float32, kv_blocks=8, speculative=4)
        assert e.speculative == 0 and e.drafter is None
        assert "speculative ignored" in capsys.readouterr().out


def test_server_main_reads_the_knobs(monkeypatch):
    from runbooks_amd.workloads import server_main
    monkeypatch.setenv("PARAM_SPECULATIVE", "4")
    monkeypatch.setenv("SPEC_NGRAM", "2")
    assert server_main._env("SPECULATIVE") == "4"
    assert server_main._env("SPEC_NGRAM") == "2"
    import inspect
    src = inspect.getsource(server_main.main)
    assert "speculative=spec_k or None" in src
    assert "spec_ngram=spec_n or None" in src


# -- streaming ----------------------------------------------------------------
def _stream_case(model):
    from runbooks_amd.serve import ByteTokenizer
    tok = ByteTokenizer()
    prompt = "abcabcabcabc"
    ref = _engine(model, batch_sampler=True)
    want = ref.generate(tok.encode(prompt), max_new_tokens=16)

    class ById:
        def propose(self, req, k):
            n = len(req.output_ids)
            return want[n:n + k]

    return tok, prompt, want, _engine(model, speculative=4, drafter=ById())


def test_engine_loop_delivers_every_token_once(model):
    """Several tokens appear per engine step; the loop that feeds the HTTP
    streams must hand each to the watcher exactly once and in order. Needs
    no web framework."""
    from runbooks_amd.serve.loop import EngineLoop

    tok, prompt, want, eng = _stream_case(model)
    loop = EngineLoop(eng)
    try:
        q, _ = loop.submit(tok.encode(prompt), 16, 0.0)
        got = []
        while True:
            t = q.get(timeout=60)
            if t is None:
                break
            got.append(t)
    finally:
        loop.shutdown()
    assert got == want
    assert eng.stats["spec_accepted"] > 0 and eng.stats["steps"] < 16


def test_http_streaming_delivers_every_token_once(model):
    """The same through the HTTP API's server-sent events."""
    pytest.importorskip("fastapi")
    import json

    from fastapi.testclient import TestClient

    from runbooks_amd.serve.http import build_app

    tok, prompt, want, eng = _stream_case(model)
    app = build_app(eng, tok, model_name="smoke-llama")
    with TestClient(app) as c:
        with c.stream("POST", "/v1/completions",
                      json={"prompt": prompt, "max_tokens": 16,
                            "stream": True}) as resp:
            assert resp.status_code == 200
            text = ""
            for line in resp.iter_lines():
                if not line or not line.startswith("data:"):
                    continue
                data = line[5:].strip()
                if data == "[DONE]":
                    break
                text += json.loads(data)["choices"][0]["text"]
    assert text == tok.decode(want)
    assert eng.stats["spec_accepted"] > 0
    assert eng.stats["steps"] < 16


# -- graph staging ------------------------------------------------------------
def test_graphed_verify_staging():
    """GraphedDecoder._stage_verify pads rows and sequences and refuses
    values the kernels would index with (the GPU-independent part of the
    verify graph family)."""
    from runbooks_amd.serve.graph import GraphedDecoder

    caches = [(torch.zeros(100, 1, BS, 8), torch.zeros(100, 1, BS, 8))]
    gd = GraphedDecoder(model=None, caches=caches, max_batch=4, max_blocks=3,
                        dummy_block=99, device="cpu")
    gd.enable_verify(3, vocab_size=512)
    ok = dict(token_rows=[[7, 8, 9], [5]], pos_rows=[[17, 18, 19], [2]],
              slot_rows=[[33, 34, 35], [66]], block_rows=[[1, 2], [4]],
              seq_lens=[20, 3])
    gd._stage_verify(4, **ok)
    h = gd.h_verify
    assert h[0:12].view(4, 3).tolist() == [[7, 8, 9], [5, 0, 0], [0] * 3,
                                           [0] * 3]
    assert h[12:24].view(4, 3).tolist() == [[17, 18, 19], [2, 2, 2], [0] * 3,
                                            [0] * 3]
    d = 99 * BS
    assert h[24:36].view(4, 3).tolist() == [[33, 34, 35], [66, d, d],
                                            [d] * 3, [d] * 3]
    assert h[36:40].tolist() == [20, 3, 0, 0]        # seq_lens
    assert h[40:44].tolist() == [3, 1, 0, 0]         # q_lens
    assert h[44:56].view(4, 3).tolist() == [[1, 2, 99], [4, 99, 99],
                                            [99] * 3, [99] * 3]
    for bad in (dict(token_rows=[[1] * 4, [5]]),            # more than T rows
                dict(token_rows=[[7, 512, 9], [5]]),        # token id
                dict(token_rows=[[7, 8, 9], [-1]]),         # token id
                dict(seq_lens=[33, 3]),                     # past its blocks
                dict(seq_lens=[2, 3]),                      # fewer keys than rows
                dict(block_rows=[[1, 100], [4]]),           # block id
                dict(slot_rows=[[33, 34, 1600], [66]]),     # slot
                dict(block_rows=[[1, 2, 3, 5], [4]])):      # wider than table
        with pytest.raises(ValueError):
            gd._stage_verify(4, **{**ok, **bad})
