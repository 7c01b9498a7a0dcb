"""Int4-resident serving (load_in_4bit + w4_resident) on the GPU: prefill
and decode on the same int4 weights, the masters' memory actually freed,
engine equality with the masters-kept int4-prefill path, the refusals of
everything that would read a released master, and tied embeddings."""
import pytest
import torch

from runbooks_amd import ops
from runbooks_amd.models import build_model
from runbooks_amd.models.transformer import (fuse_for_inference,
                                             release_w4_masters)
from runbooks_amd.ops import linear as L
from runbooks_amd.serve import Engine

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PROMPT40 = [(7 * i + 3) % 500 + 1 for i in range(40)]


@pytest.fixture(autouse=True)
def _clean_registries(monkeypatch):
    monkeypatch.delenv("RB_W4_PREFILL", raising=False)
    monkeypatch.delenv("RB_W4_RESIDENT", raising=False)
    L._W4_REGISTRY.clear()
    L._W4_RELEASED.clear()
    yield
    L._W4_REGISTRY.clear()
    L._W4_RELEASED.clear()


def _w4_weights(model):
    out = []
    for blk in model.blocks:
        out += [blk.attn._qkv_w, blk.mlp._gateup_w, blk.attn.o_proj.weight,
                blk.mlp.down_proj.weight]
    return out + [model.lm_head.weight]


def _views(model):
    out = []
    for blk in model.blocks:
        out += [blk.attn.q_proj.weight, blk.attn.k_proj.weight,
                blk.attn.v_proj.weight, blk.mlp.gate_proj.weight,
                blk.mlp.up_proj.weight]
    return out


def test_prefill_and_decode_on_the_same_int4_weights():
    """A resident 4-bit model against a bf16 model of the same seed whose
    weights went through fake_quantize_int4_: a 40-token prefill (M > 32,
    csrc/gemm_w4.hip) and one decode step, both within 3e-2 of max, the
    metric and tolerance of
    test_w4_gpu.test_4bit_decode_logits_match_fake_quantized_bf16. The
    4-bit model is not touched by hand: it has no masters left to edit."""
    assert ops.has_hip()
    m4 = build_model("smoke-llama", dtype=torch.bfloat16, device=DEV,
                     seed=11)
    fuse_for_inference(m4, load_in_4bit=True, w4_resident=True)
    for w in _w4_weights(m4):
        assert w.device.type == "meta" and L.w4_registered(w)

    ref = build_model("smoke-llama", dtype=torch.bfloat16, device=DEV,
                      seed=11)
    # per row and per 64-group of K, so quantizing the projections one by
    # one equals quantizing the fused weights; done before fusing, so any
    # decode-layout copy is taken from the quantized values
    for blk in ref.blocks:
        for lin in (blk.attn.q_proj, blk.attn.k_proj, blk.attn.v_proj,
                    blk.attn.o_proj, blk.mlp.gate_proj, blk.mlp.up_proj,
                    blk.mlp.down_proj):
            L.fake_quantize_int4_(lin.weight.data)
    L.fake_quantize_int4_(ref.lm_head.weight.data)
    fuse_for_inference(ref)
    for w in _w4_weights(ref):
        assert not L.w4_registered(w)

    S = len(PROMPT40)

    def run(model):
        caches = model.alloc_caches(8, DEV)
        tokens = torch.tensor([PROMPT40], dtype=torch.long, device=DEV)
        pos = torch.arange(S, dtype=torch.int32, device=DEV)
        slots = torch.arange(S, dtype=torch.int32, device=DEV)
        lp = model.prefill(tokens, pos, caches, slots)
        t = torch.tensor([3], dtype=torch.long, device=DEV)
        p = torch.tensor([S], dtype=torch.int32, device=DEV)
        sl = torch.tensor([S], dtype=torch.int32, device=DEV)
        bt = torch.tensor([[0, 1, 2]], dtype=torch.int32, device=DEV)
        seq = torch.tensor([S + 1], dtype=torch.int32, device=DEV)
        ld = model.decode(t, p, caches, sl, bt, seq)
        return lp.float().cpu(), ld.float().cpu()

    with torch.no_grad():
        lp4, ld4 = run(m4)
        lpr, ldr = run(ref)
    for name, got, want in (("prefill", lp4, lpr), ("decode", ld4, ldr)):
        scale = want.abs().max().item()
        err = (got - want).abs().max().item() / scale
        print(f"w4 resident {name} logits rel err {err:.3e}")
        assert err < 3e-2, (name, err, got[:, :8], want[:, :8])


def test_release_frees_the_masters():
    assert ops.has_hip()
    m = build_model("smoke-llama", dtype=torch.bfloat16, device=DEV, seed=2)
    fuse_for_inference(m, load_in_4bit=True)
    ws = _w4_weights(m)
    shapes = [tuple(w.shape) for w in ws]
    view_shapes = [tuple(w.shape) for w in _views(m)]
    want = sum(w.numel() * w.element_size() for w in ws)
    assert len(L._W4_REGISTRY) == len(ws) == 9
    del ws
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    released = release_w4_masters(m)
    torch.cuda.synchronize()
    after = torch.cuda.memory_allocated()
    print(f"release_w4_masters: {want} master bytes, allocated "
          f"{before} -> {after}")
    assert released == want
    assert before - after >= 0.95 * want, (before, after, want)
    ws = _w4_weights(m)
    assert [tuple(w.shape) for w in ws] == shapes
    assert [tuple(w.shape) for w in _views(m)] == view_shapes
    for w in ws:
        assert w.dtype == torch.bfloat16 and w.device.type == "meta"
        assert L.w4_registered(w)
    for w in _views(m):
        assert w.device.type == "meta" and not L.w4_registered(w)
    assert not L._W4_REGISTRY and L.w4_prefill_enabled()
    # the embedding is no int4 weight: it stays
    assert m.embed.weight.is_cuda


@pytest.mark.parametrize("chunk", [0, 16])
def test_engine_resident_equals_masters_kept(chunk, monkeypatch):
    """The resident engine and one that keeps its masters but has
    RB_W4_PREFILL on run the same kernels on the same int4 copies: greedy
    generation from a 40-token prompt is identical, whole-prompt and with
    prefill_chunk=16, under hipGraph decode."""
    assert ops.has_hip()
    kw = dict(device=DEV, kv_blocks=128, seed=11, load_in_4bit=True,
              prefill_chunk=chunk)
    res = Engine(build_model("smoke-llama", dtype=torch.bfloat16, seed=4),
                 w4_resident=True, **kw)
    assert res.w4_resident and res.use_graphs
    assert not L._W4_REGISTRY and len(L._W4_RELEASED) == 9 + 10
    out_res = res.generate(list(PROMPT40), max_new_tokens=8)
    if chunk:
        assert res.stats["prefill_chunks"] == 3
    del res
    L._W4_RELEASED.clear()

    monkeypatch.setenv("RB_W4_PREFILL", "1")
    keep = Engine(build_model("smoke-llama", dtype=torch.bfloat16, seed=4),
                  **kw)
    assert not keep.w4_resident and keep.use_graphs
    assert len(L._W4_REGISTRY) == 9 and not L._W4_RELEASED
    assert keep.model.lm_head.weight.is_cuda
    out_keep = keep.generate(list(PROMPT40), max_new_tokens=8)
    assert len(out_res) == 8
    assert out_res == out_keep, (out_res, out_keep)


def test_touching_a_released_master_raises():
    assert ops.has_hip()
    m = build_model("smoke-llama", dtype=torch.bfloat16, device=DEV, seed=5)
    fuse_for_inference(m, load_in_4bit=True, w4_resident=True)
    w = m.blocks[1].attn.o_proj.weight
    with torch.no_grad():
        # the F.linear path: fp32 input, and a bias
        with pytest.raises(RuntimeError, match="int4-resident") as ei:
            ops.fast_linear(torch.randn(4, w.shape[1], device=DEV), w)
        assert "blocks.1.attn.o_proj.weight" in str(ei.value)
        xb = torch.randn(4, w.shape[1], device=DEV).to(torch.bfloat16)
        with pytest.raises(RuntimeError, match="int4-resident"):
            ops.fast_linear(xb, w, torch.zeros(w.shape[0], device=DEV,
                                               dtype=torch.bfloat16))
        # a per-projection view has no int4 copy of its own
        with pytest.raises(RuntimeError, match="q_proj.weight"):
            ops.fast_linear(xb, m.blocks[0].attn.q_proj.weight)
        assert ops.fast_linear(xb, w).shape == (4, w.shape[0])
    with pytest.raises(RuntimeError, match="int4-resident"):
        m.state_dict()
    with pytest.raises(RuntimeError, match="int4-resident"):
        L.register_decode_weight(w)
    tokens = torch.randint(0, 512, (1, 8), device=DEV)
    with torch.enable_grad():
        with pytest.raises(RuntimeError, match="int4-resident"):
            m(tokens)


def test_tied_embedding_keeps_its_master():
    assert ops.has_hip()
    eng = Engine(build_model("smoke-gemma", dtype=torch.bfloat16, seed=6),
                 device=DEV, kv_blocks=128, seed=1, load_in_4bit=True,
                 w4_resident=True)
    m = eng.model
    assert eng.w4_resident
    assert m.lm_head.weight is m.embed.weight and m.embed.weight.is_cuda
    assert L.w4_registered(m.lm_head.weight)      # decode still streams int4
    assert m.blocks[0].attn.o_proj.weight.device.type == "meta"
    out = eng.generate(list(PROMPT40), max_new_tokens=4)
    assert len(out) == 4 and all(0 <= t < m.cfg.vocab_size for t in out)
