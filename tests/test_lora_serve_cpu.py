"""Serving many LoRA adapters over one base model, on the CPU reference
path: the two per-row ops, the adapter pool, the model entry points'
``lora=`` argument, the engine (mixed batches, prefix cache) and the HTTP
``model`` field."""
import copy
import json

import pytest
import torch

from runbooks_amd import ops
from runbooks_amd.models import build_model
from runbooks_amd.models.transformer import fuse_for_inference
from runbooks_amd.serve import Engine
from runbooks_amd.serve.lora import AdapterPool, LoraBatch
from runbooks_amd.train.checkpoint import save_checkpoint
from runbooks_amd.train.lora import apply_lora, lora_state_dict, merge_lora

TARGETS = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj",
           "down_proj")


# ---------------------------------------------------------------------------
# op references
# ---------------------------------------------------------------------------
IDX = [1, -1, 3, 1, 0, -1, 2]


def _seg_of(N, seg_ends):
    seg = torch.zeros(N, dtype=torch.long)
    for e in seg_ends[:-1]:
        seg += (torch.arange(N) >= e).long()
    return seg


@pytest.mark.parametrize("S,R", [(1, 16), (2, 16), (3, 16), (1, 64)])
def test_shrink_ref_matches_fp64_einsum(S, R):
    g = torch.Generator().manual_seed(S * 100 + R)
    M, K, slots = len(IDX), 72, 4
    x = torch.randn(M, K, generator=g)
    a = torch.randn(slots, S * R, K, generator=g)
    idx = torch.tensor(IDX, dtype=torch.int32)
    t = ops.lora_shrink(x, a, idx, segments=S)
    assert t.dtype == torch.float32 and t.shape == (M, S * R)
    ref = torch.einsum("mk,mjk->mj", x.double(),
                       a[idx.clamp_min(0).long()].double())
    ref[idx < 0] = 0
    assert (t[idx < 0] == 0).all()
    bound = K * 2.0 ** -23 * torch.einsum(
        "mk,mjk->mj", x.double().abs(),
        a[idx.clamp_min(0).long()].double().abs())
    assert ((t.double() - ref).abs() <= bound + 1e-30).all()


@pytest.mark.parametrize("N,seg_ends,R", [
    (256, (256,), 16), (512, (256, 384, 512), 16),
    (1000, (424, 1000), 16),        # boundary not a multiple of 256
    (256, (256,), 64)])
def test_expand_ref_matches_fp64_einsum(N, seg_ends, R):
    g = torch.Generator().manual_seed(N + R)
    M, slots, S = len(IDX), 4, len(seg_ends)
    y0 = torch.randn(M, N, generator=g)
    t = torch.randn(M, S * R, generator=g)
    b = torch.randn(slots, N, R, generator=g)
    sc = torch.rand(slots, generator=g) + 0.5
    idx = torch.tensor(IDX, dtype=torch.int32)
    y = ops.lora_expand_(y0.clone(), t, b, sc, idx, seg_ends)
    seg = _seg_of(N, seg_ends)
    tj = t.double().view(M, S, R)[:, seg]                       # [M, N, R]
    bj = b[idx.clamp_min(0).long()].double()
    ref = y0.double() + sc[idx.clamp_min(0).long()].double()[:, None] * \
        (tj * bj).sum(-1)
    live = idx >= 0
    assert torch.equal(y[~live], y0[~live])                     # untouched
    mag = y0.double().abs() + sc[idx.clamp_min(0).long()].double()[:, None] \
        * (tj * bj).abs().sum(-1)
    assert ((y.double() - ref).abs()[live] <=
            (R + 2) * 2.0 ** -23 * mag[live]).all()


def test_op_wrappers_check_their_arguments():
    x = torch.zeros(2, 16)
    a = torch.zeros(2, 16, 16)
    idx = torch.tensor([0, 2], dtype=torch.int32)
    with pytest.raises(ValueError, match="idx\\[1\\] = 2"):
        ops.lora_shrink(x, a, idx)
    ok = torch.tensor([0, -1], dtype=torch.int32)
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.lora_shrink(torch.zeros(2, 12), torch.zeros(2, 16, 12), ok)
    with pytest.raises(ValueError, match="rank"):
        ops.lora_shrink(x, torch.zeros(2, 24, 16), ok)
    t = torch.zeros(2, 16)
    b = torch.zeros(2, 32, 16)
    sc = torch.ones(2)
    with pytest.raises(ValueError, match="seg_ends"):
        ops.lora_expand_(torch.zeros(2, 32), t, b, sc, ok, (16, 24))
    with pytest.raises(ValueError, match="idx_cpu|idx\\["):
        ops.lora_expand_(torch.zeros(2, 32), t, b, sc, ok, (32,),
                         idx_cpu=[0, 5])


# ---------------------------------------------------------------------------
# adapters for smoke-llama, the apply_lora reference
# ---------------------------------------------------------------------------
SEED = 3


def _random_adapter(seed, r=16, b_std=0.05, dtype=torch.float32,
                    targets=TARGETS):
    """State dict of a random adapter in the trainer's own layout."""
    ref = build_model("smoke-llama", dtype=dtype, seed=SEED)
    apply_lora(ref, r=r, alpha=32, targets=targets)
    g = torch.Generator().manual_seed(seed)
    state = {}
    for k, v in lora_state_dict(ref).items():
        std = b_std if k.endswith("lora_b") else 0.05
        state[k] = (torch.randn(v.shape, generator=g) * std).to(dtype)
    return state


def _reference_model(state, dtype, r=16):
    """The formulation the trainer runs: base wrapped by apply_lora."""
    ref = build_model("smoke-llama", dtype=torch.float32, seed=SEED).to(dtype)
    if state is not None:
        apply_lora(ref, r=r, alpha=32)
        missing, unexpected = ref.load_state_dict(
            {k: v.to(dtype) for k, v in state.items()}, strict=False)
        assert not unexpected
    return ref.eval()


PROMPT = [5, 9, 2, 7, 11]


def _prefill_decode(model, n_seq, lora_p=None, lora_d=None):
    """Prefill n_seq copies of PROMPT (sequence b in block b), then one
    decode step for all of them. Returns (prefill, decode) logits."""
    S = len(PROMPT)
    caches = model.alloc_caches(4, "cpu")
    tokens = torch.tensor([PROMPT] * n_seq, dtype=torch.long)
    pos = torch.arange(S, dtype=torch.int32).repeat(n_seq)
    slots = torch.cat([torch.arange(S, dtype=torch.int32) + b * ops.BLOCK_SIZE
                       for b in range(n_seq)])
    kw = {} if lora_p is None else {"lora": lora_p}
    lp = model.prefill(tokens, pos, caches, slots, **kw)
    kw = {} if lora_d is None else {"lora": lora_d}
    ld = model.decode(
        torch.full((n_seq,), 3, dtype=torch.long),
        torch.full((n_seq,), S, dtype=torch.int32), caches,
        torch.tensor([b * ops.BLOCK_SIZE + S for b in range(n_seq)],
                     dtype=torch.int32),
        torch.arange(n_seq, dtype=torch.int32).view(n_seq, 1),
        torch.full((n_seq,), S + 1, dtype=torch.int32), **kw)
    return lp, ld


@pytest.fixture(scope="module")
def adapters():
    return {"A": _random_adapter(101), "B": _random_adapter(202)}


@pytest.fixture(scope="module")
def references(adapters):
    """name -> (fp32 logits, fp64 logits) of the apply_lora reference,
    computed once; [prefill, decode] stacked."""
    out = {}
    for name, state in (("none", None), ("A", adapters["A"]),
                        ("B", adapters["B"])):
        pair = []
        for dt in (torch.float32, torch.float64):
            with torch.no_grad():
                lp, ld = _prefill_decode(_reference_model(state, dt), 1)
            pair.append(torch.cat([lp, ld]).double())
        out[name] = tuple(pair)
    return out


def test_model_lora_matches_apply_lora_reference(adapters, references):
    """prefill + one decode with ``lora=`` (rows: none, A, B) against the
    same base wrapped by apply_lora. Tolerance: 10x the fp32 reference's
    own deviation from the fp64 run of it (the norm and rope references
    round to fp32 inside, in both runs; GEMMs, attention and the residual
    stream run in fp64). The references must differ pairwise by >= 100x
    that tolerance, or a path that ignored ``idx`` would pass."""
    m = fuse_for_inference(build_model("smoke-llama", dtype=torch.float32,
                                       seed=SEED)).eval()
    pool = AdapterPool(m, max_loras=2, rank=16)
    pool.load_state("A", adapters["A"], alpha=32)
    pool.load_state("B", adapters["B"], alpha=32)
    rows = [-1, pool.slot_of("A"), pool.slot_of("B")]
    lp, ld = _prefill_decode(m, 3, LoraBatch(pool, rows),
                             LoraBatch(pool, rows))
    own = max((references[n][0] - references[n][1]).abs().max().item()
              for n in references)
    tol = 10 * own
    print(f"fp32 reference deviation {own:.3e}, tolerance {tol:.3e}")
    names = ["none", "A", "B"]
    for i, n in enumerate(names):
        got = torch.stack([lp[i], ld[i]]).double()
        err = (got - references[n][1]).abs().max().item()
        print(f"row {n}: max error vs fp64 {err:.3e}")
        assert err <= tol, (n, err, tol)
    for i in range(3):
        for j in range(i + 1, 3):
            sep = (references[names[i]][1] -
                   references[names[j]][1]).abs().max().item()
            print(f"separation {names[i]}/{names[j]}: {sep:.3e}")
            assert sep >= 100 * tol, (names[i], names[j], sep, tol)


# ---------------------------------------------------------------------------
# AdapterPool.load
# ---------------------------------------------------------------------------
@pytest.fixture()
def pool():
    m = fuse_for_inference(build_model("smoke-llama", dtype=torch.float32,
                                       seed=SEED))
    return AdapterPool(m, max_loras=2, rank=16)


def _same_slot(pool, name, state, r=16, alpha=32.0):
    slot = pool.slot_of(name)
    R = pool.rank
    assert pool.scale_host[slot] == alpha / r
    assert float(pool.scales[slot]) == alpha / r
    qkv = pool.sites[1]["qkv"]
    for s, tgt in enumerate(("q_proj", "k_proj", "v_proj")):
        a = state[f"blocks.1.attn.{tgt}.lora_a"]
        b = state[f"blocks.1.attn.{tgt}.lora_b"]
        lo = qkv.seg_ends[s - 1] if s else 0
        assert torch.equal(qkv.a[slot, s * R:s * R + r], a)
        assert (qkv.a[slot, s * R + r:(s + 1) * R] == 0).all()
        assert torch.equal(qkv.b[slot, lo:qkv.seg_ends[s], :r], b)
        assert (qkv.b[slot, lo:qkv.seg_ends[s], r:] == 0).all()
    down = pool.sites[0]["down"]
    assert torch.equal(down.b[slot, :, :r],
                       state["blocks.0.mlp.down_proj.lora_b"])


def test_pool_loads_trainer_checkpoint(pool, adapters, tmp_path):
    save_checkpoint(tmp_path / "run", 7, adapters["A"])
    save_checkpoint(tmp_path / "run", 12, adapters["B"])
    pool.load("old", tmp_path / "run" / "checkpoint-7")
    pool.load("latest", tmp_path / "run")      # picks checkpoint-12
    _same_slot(pool, "old", adapters["A"])
    _same_slot(pool, "latest", adapters["B"])
    assert pool.loaded() == ["old", "latest"]
    with pytest.raises(RuntimeError, match="slots are in use"):
        pool.load("third", tmp_path / "run")
    pool.unload("old")
    (tmp_path / "run" / "checkpoint-12" / "adapter.json").write_text(
        json.dumps({"lora_alpha": 8, "lora_r": 16}))
    pool.load("third", tmp_path / "run")
    _same_slot(pool, "third", adapters["B"], alpha=8.0)


def test_pool_loads_peft_directory(pool, adapters, tmp_path):
    from safetensors.torch import save_file
    hf = {}
    for k, v in adapters["A"].items():
        i, grp, tgt, kind = k.split(".")[1:]
        hf_grp = "self_attn" if grp == "attn" else "mlp"
        hf[f"base_model.model.model.layers.{i}.{hf_grp}.{tgt}."
           f"lora_{kind[-1].upper()}.weight"] = v
    d = tmp_path / "peft"
    d.mkdir()
    save_file(hf, str(d / "adapter_model.safetensors"))
    (d / "adapter_config.json").write_text(json.dumps(
        {"r": 16, "lora_alpha": 64, "peft_type": "LORA"}))
    pool.load("p", d)
    _same_slot(pool, "p", adapters["A"], alpha=64.0)


def test_pool_zero_pads_a_smaller_rank(pool):
    small = _random_adapter(7, r=8)
    pool.load_state("r8", small, alpha=32)
    _same_slot(pool, "r8", small, r=8)
    # a lacking target stays zero
    few = _random_adapter(8, targets=("q_proj", "down_proj"))
    pool.load_state("few", few, alpha=32)
    slot = pool.slot_of("few")
    assert (pool.sites[0]["gateup"].a[slot] == 0).all()
    assert (pool.sites[0]["qkv"].b[slot, 256:] == 0).all()
    assert pool.sites[0]["qkv"].b[slot, :256].abs().sum() > 0


def test_pool_refusals_name_the_offender(pool, adapters):
    big = _random_adapter(9, r=32)
    with pytest.raises(ValueError, match="'big'.*rank 32"):
        pool.load_state("big", big, alpha=32)
    bad = dict(adapters["A"])
    bad["blocks.0.attn.o_proj.lora_b"] = torch.zeros(100, 16)
    with pytest.raises(ValueError, match="'bad'.*o_proj.*do not match"):
        pool.load_state("bad", bad, alpha=32)
    odd = dict(adapters["A"])
    odd["blocks.0.mlp.fc1.lora_a"] = torch.zeros(16, 256)
    odd["blocks.0.mlp.fc1.lora_b"] = torch.zeros(512, 16)
    with pytest.raises(ValueError, match="'odd'.*blocks.0.mlp.fc1"):
        pool.load_state("odd", odd, alpha=32)
    head = dict(adapters["A"])
    head["lm_head.lora_a"] = torch.zeros(16, 256)
    with pytest.raises(ValueError, match="'head'.*lm_head"):
        pool.load_state("head", head, alpha=32)
    assert pool.loaded() == []          # refused adapters leave no trace
    with pytest.raises(ValueError, match="multiple of 16"):
        AdapterPool(pool.model, 2, rank=24)
    with pytest.raises(NotImplementedError, match="fused qkv"):
        AdapterPool(build_model("smoke-llama", dtype=torch.float32), 2)


# ---------------------------------------------------------------------------
# engine
# ---------------------------------------------------------------------------
def _engine(adapters, max_loras=2, **kw):
    eng = Engine(build_model("smoke-llama", dtype=torch.float32, seed=SEED),
                 device="cpu", dtype=torch.float32, kv_blocks=64, seed=5,
                 max_loras=max_loras, **kw)
    if max_loras:
        for name, state in adapters.items():
            eng.lora_pool.load_state(name, state, alpha=32)
    return eng


def _run(eng, reqs):
    while not all(r.finished for r in reqs):
        eng.step()
    return [r.output_ids for r in reqs]


def _merged_tokens(state, prompt, n):
    ref = build_model("smoke-llama", dtype=torch.float32, seed=SEED)
    if state is not None:
        apply_lora(ref, r=16, alpha=32)
        ref.load_state_dict(state, strict=False)
        merge_lora(ref)
        for blk in ref.blocks:      # unwrap: serve the merged base weights
            for mod in (blk.attn, blk.mlp):
                for n_, child in list(mod.named_children()):
                    if hasattr(child, "lora_a"):
                        setattr(mod, n_, child.base)
    eng = Engine(ref, device="cpu", dtype=torch.float32, kv_blocks=64, seed=5)
    return eng.generate(list(prompt), max_new_tokens=n)


def test_engine_mixed_batch_matches_merged_models(adapters):
    """One engine, one batch, rows (none, A, B, A): each request decodes
    what a server of the merged fine-tune would."""
    eng = _engine(adapters)
    prompts = [[1, 2, 3, 4], [5, 6, 7], [1, 2, 3, 4], [9, 8, 7, 6, 5]]
    names = [None, "A", "B", "A"]
    reqs = [eng.submit(p, max_new_tokens=6, adapter=a)
            for p, a in zip(prompts, names)]
    got = _run(eng, reqs)
    for p, a, out in zip(prompts, names, got):
        want = _merged_tokens(adapters.get(a), p, 6)
        assert out == want, (a, out, want)
    assert eng.stats["lora_decode_steps"] > 0
    assert eng.stats["lora_rows"] >= 3 * 4
    assert got[0] != got[2]             # same prompt, base vs B
    with pytest.raises(KeyError):
        eng.submit([1, 2], adapter="nope")
    assert eng.adapters() == ["A", "B"]


def test_engine_unload_refused_while_in_use(adapters):
    eng = _engine(adapters)
    r = eng.submit([1, 2, 3], max_new_tokens=3, adapter="A")
    with pytest.raises(RuntimeError, match="in use"):
        eng.unload_adapter("A")         # waiting
    eng.step()
    with pytest.raises(RuntimeError, match="in use"):
        eng.unload_adapter("A")         # running
    _run(eng, [r])
    eng.unload_adapter("A")
    assert eng.adapters() == ["B"]
    with pytest.raises(KeyError):
        eng.submit([1], adapter="A")
    with pytest.raises(KeyError):
        eng.unload_adapter("A")


@pytest.mark.parametrize("mode", ["default", "from_cache", "batch"])
def test_prefix_cache_is_per_adapter(adapters, mode):
    kw = {"default": {}, "from_cache": {"prefill_from_cache": True},
          "batch": {"prefill_from_cache": True, "prefill_batch": 2}}[mode]
    eng = _engine(adapters, prefix_cache=True, **kw)
    prompt = list(range(1, 36))          # two full blocks + a tail

    def serve(adapter):
        r = eng.submit(prompt, max_new_tokens=3, adapter=adapter)
        eng.step()
        blocks = list(r.blocks[:2])
        _run(eng, [r])
        return blocks, r.output_ids

    a_blocks, a_out = serve("A")
    assert eng.stats["prefix_hits"] == 0
    b_blocks, b_out = serve("B")
    assert eng.stats["prefix_hits"] == 0, "hit across adapters"
    n_blocks, n_out = serve(None)
    assert eng.stats["prefix_hits"] == 0, "base hit on an adapter's blocks"
    assert not set(a_blocks) & set(b_blocks)
    assert not (set(a_blocks) | set(b_blocks)) & set(n_blocks)
    a2_blocks, a2_out = serve("A")
    assert eng.stats["prefix_hits"] == 1 and a2_blocks == a_blocks
    assert a2_out == a_out
    assert b_out == _merged_tokens(adapters["B"], prompt, 3)
    assert a_out == _merged_tokens(adapters["A"], prompt, 3)
    assert n_out == _merged_tokens(None, prompt, 3)


def test_engine_with_idle_pool_matches_plain_engine(adapters):
    prompts = [[1, 2, 3, 4], [7, 7, 2]]
    plain = _engine(adapters, max_loras=0)
    assert plain.lora_pool is None and "lora_rows" not in plain.stats
    want = _run(plain, [plain.submit(p, max_new_tokens=8) for p in prompts])
    eng = _engine(adapters, max_loras=2)
    got = _run(eng, [eng.submit(p, max_new_tokens=8) for p in prompts])
    assert got == want
    assert eng.stats["lora_decode_steps"] == 0
    with pytest.raises(RuntimeError, match="max_loras"):
        plain.load_adapter("x", "/nonexistent")
    with pytest.raises(KeyError):
        plain.submit([1], adapter="A")


def test_preemption_keeps_the_adapter(adapters):
    eng = _engine(adapters)
    r = eng.submit([1, 2, 3, 4], max_new_tokens=6, adapter="B")
    eng.step()
    eng.step()
    eng._preempt(r)
    assert r.adapter == "B"
    _run(eng, [r])
    full = r.prompt_ids[4:] + r.output_ids
    assert full == _merged_tokens(adapters["B"], [1, 2, 3, 4], 6)


def test_engine_refuses_unsupported_models():
    with pytest.raises(NotImplementedError, match="tiny-falcon"):
        Engine("tiny-falcon", device="cpu", dtype=torch.float32,
               kv_blocks=32, max_loras=1)
    with pytest.raises(NotImplementedError, match="fp8"):
        Engine("smoke-llama", device="cpu", dtype=torch.float32,
               kv_blocks=32, max_loras=1, kv_fp8=True)


# ---------------------------------------------------------------------------
# HTTP
# ---------------------------------------------------------------------------
def test_http_model_field_selects_the_adapter(adapters, tmp_path):
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient

    from runbooks_amd.serve.http import build_app
    eng = _engine({})
    app = build_app(eng, model_name="base")
    save_checkpoint(tmp_path / "a", 1, adapters["A"])
    save_checkpoint(tmp_path / "b", 1, adapters["B"])
    with TestClient(app) as c:
        loop = app.state.engine_loop
        loop.load_adapter("a", tmp_path / "a")       # on the engine thread
        loop.load_adapter("b", tmp_path / "b")
        listing = c.get("/v1/models").json()["data"]
        assert [m["id"] for m in listing] == ["base", "a", "b"]
        assert "parent" not in listing[0]
        assert all(m["parent"] == "base" for m in listing[1:])
        assert c.get("/v1/models/b").json()["parent"] == "base"
        assert c.get("/v1/models/zzz").status_code == 404

        def text(path="/v1/completions", **body):
            if path.endswith("chat/completions"):
                body = {"messages": [{"role": "user", "content": "hi"}],
                        **body}
            else:
                body = {"prompt": "hello", **body}
            r = c.post(path, json={"max_tokens": 6, **body})
            assert r.status_code == 200, r.text
            ch = r.json()["choices"][0]
            return r.json()["model"], ch.get("text",
                                             ch.get("message", {})
                                             .get("content"))

        rows = eng.stats["lora_rows"]
        served, base_text = text()
        assert served == "base" and eng.stats["lora_rows"] == rows
        assert text(model="base") == ("base", base_text)
        assert text(model="") == ("base", base_text)
        served_a, a_text = text(model="a")
        assert served_a == "a" and eng.stats["lora_rows"] > rows
        served_b, b_text = text(model="b")
        assert served_b == "b"
        assert len({base_text, a_text, b_text}) == 3
        rows = eng.stats["lora_rows"]
        assert text("/v1/chat/completions", model="a")[0] == "a"
        assert eng.stats["lora_rows"] > rows
        for path, body in (("/v1/completions", {"prompt": "x"}),
                           ("/v1/chat/completions",
                            {"messages": [{"role": "user",
                                           "content": "x"}]})):
            r = c.post(path, json={**body, "model": "nope"})
            assert r.status_code == 404
            assert "nope" in r.json()["error"]["message"]
        loop.unload_adapter("a")
        assert [m["id"] for m in c.get("/v1/models").json()["data"]] == \
            ["base", "b"]
        assert c.post("/v1/completions", json={
            "prompt": "x", "model": "a"}).status_code == 404


# ---------------------------------------------------------------------------
# trainer side file, pool edge cases, server workload
# ---------------------------------------------------------------------------
def test_trainer_checkpoint_carries_adapter_json(tmp_path):
    """Trainer.save writes adapter.json inside the checkpoint (before it is
    renamed into place) and the pool takes alpha / r from it."""
    from runbooks_amd.train.trainer import TrainConfig, Trainer
    cfg = TrainConfig(model="smoke-llama", dtype="float32", lora_r=8,
                      lora_alpha=24, output_dir=str(tmp_path), seq_len=8,
                      micro_batch=1)
    tr = Trainer(cfg, device="cpu")
    tr.step_num = 5
    tr.save()
    ck = tmp_path / "checkpoint-5"
    assert json.loads((ck / "adapter.json").read_text()) == \
        {"lora_alpha": 24, "lora_r": 8}
    assert not list(tmp_path.glob(".tmp-ckpt-*"))
    m = fuse_for_inference(build_model("smoke-llama", dtype=torch.float32))
    pool = AdapterPool(m, max_loras=1, rank=16)
    pool.load("mine", tmp_path)
    assert pool.scale_host[0] == 24 / 8
    full = TrainConfig(model="smoke-llama", dtype="float32",
                       full_finetune=True, output_dir=str(tmp_path / "f"),
                       seq_len=8, micro_batch=1)
    Trainer(full, device="cpu").save()
    assert not (tmp_path / "f" / "checkpoint-0" / "adapter.json").exists()


def test_pool_full_and_unsupported_shapes(pool, adapters):
    pool.load_state("A", adapters["A"], alpha=32)
    pool.load_state("B", adapters["B"], alpha=32)
    with pytest.raises(RuntimeError, match="'C'.*slots are in use"):
        pool.load_state("C", adapters["A"], alpha=32)
    import dataclasses

    from runbooks_amd.models import get_config
    odd = dataclasses.replace(get_config("smoke-llama"), name="odd-llama",
                              intermediate_size=508)
    m = fuse_for_inference(build_model(odd, dtype=torch.float32))
    with pytest.raises(NotImplementedError,
                       match="intermediate_size = 508.*multiple of 8"):
        AdapterPool(m, 1)


def test_parse_lora_adapters(tmp_path):
    from runbooks_amd.workloads.server_main import parse_lora_adapters as p
    assert p("") == [] and p(" , ") == []
    assert p("a=/x/a, b = /x/b") == [("a", tmp_path.__class__("/x/a")),
                                     ("b", tmp_path.__class__("/x/b"))]
    for n in ("sql", "bot", ".hidden"):
        (tmp_path / n).mkdir()
    (tmp_path / "notes.txt").write_text("x")
    assert p(f"z=/q,{tmp_path}") == [
        ("z", tmp_path.__class__("/q")), ("bot", tmp_path / "bot"),
        ("sql", tmp_path / "sql")]
    with pytest.raises(ValueError, match="repeated"):
        p(f"sql=/x,{tmp_path}")
    with pytest.raises(ValueError, match="empty or repeated"):
        p("=/x")
    with pytest.raises(ValueError, match="neither"):
        p(str(tmp_path / "missing"))


def test_server_main_loads_listed_adapters(adapters, tmp_path, monkeypatch):
    """LORA_ADAPTERS -> Engine(max_loras = number listed) -> load_adapter,
    before the HTTP layer starts."""
    from runbooks_amd.serve import http
    from runbooks_amd.workloads import server_main
    save_checkpoint(tmp_path / "a", 1, adapters["A"])
    save_checkpoint(tmp_path / "b", 3, adapters["B"])
    seen = {}

    def fake_serve(engine, tok, port=8080, model_name="model"):
        seen.update(engine=engine, model_name=model_name)

    monkeypatch.setattr(http, "serve_forever", fake_serve)
    for k in ("TP", "RANK", "MAX_LORAS", "PARAM_MAX_LORAS", "LORA_RANK",
              "PARAM_LORA_RANK", "LORA_ADAPTERS", "RB_MAX_LORAS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MODEL_DIR", str(tmp_path / "no-model"))
    monkeypatch.setenv("PARAM_MODEL", "smoke-llama")
    monkeypatch.setenv("PARAM_LORA_ADAPTERS",
                       f"a={tmp_path / 'a'},b={tmp_path / 'b'}")
    assert server_main.main() == 0
    eng = seen["engine"]
    assert eng.max_loras == 2 and eng.lora_rank == 16
    assert eng.adapters() == ["a", "b"] and seen["model_name"] == "smoke-llama"
    monkeypatch.delenv("PARAM_LORA_ADAPTERS")
    assert server_main.main() == 0
    assert seen["engine"].lora_pool is None
