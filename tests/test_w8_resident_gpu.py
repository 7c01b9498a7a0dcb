"""Fp8-resident serving (load_in_8bit + w8_resident) on the GPU."""
import pytest
import torch

from runbooks_amd import ops
from runbooks_amd.models import build_model
from runbooks_amd.models.transformer import (fuse_for_inference,
                                             release_w8_masters)
from runbooks_amd.ops import linear as L
from runbooks_amd.serve import Engine

from test_w4_resident_gpu import PROMPT40, _views, _w4_weights as _weights

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _clean_registries(monkeypatch):
    monkeypatch.setenv("RB_DECODE_GEMM_W8", "1")
    monkeypatch.delenv("RB_W8_PREFILL", raising=False)
    monkeypatch.delenv("RB_W8_RESIDENT", raising=False)
    L._FP8_REGISTRY.clear()
    L._W8_RELEASED.clear()
    yield
    L._FP8_REGISTRY.clear()
    L._W8_RELEASED.clear()


def test_release_frees_the_masters():
    m = build_model("smoke-llama", dtype=torch.bfloat16, device=DEV, seed=2)
    fuse_for_inference(m, load_in_8bit=True)
    ws = _weights(m)
    shapes = [tuple(w.shape) for w in ws + _views(m)]
    want = sum(w.numel() * w.element_size() for w in ws)
    assert len(L._FP8_REGISTRY) == len(ws) == 9
    del ws
    before = torch.cuda.memory_allocated()
    released = release_w8_masters(m)
    after = torch.cuda.memory_allocated()
    assert released == want
    assert before - after >= 0.95 * want, (before, after, want)
    assert [tuple(w.shape) for w in _weights(m) + _views(m)] == shapes
    for w in _weights(m):
        assert w.dtype == torch.bfloat16 and w.device.type == "meta"
        assert L._w8_get(w) is not None
    for w in _views(m):
        assert w.device.type == "meta" and L._w8_get(w) is None
    assert not L._FP8_REGISTRY and L.w8_prefill_enabled()
    assert m._w8_resident and m.embed.weight.is_cuda


@pytest.mark.parametrize("chunk", [0, 16])
def test_engine_resident_equals_masters_kept(chunk, monkeypatch):
    """Resident and masters-kept + RB_W8_PREFILL run the same kernels on
    the same fp8 copies: identical greedy tokens, under hipGraph decode."""
    kw = dict(device=DEV, kv_blocks=128, seed=11, load_in_8bit=True,
              prefill_chunk=chunk)
    res = Engine(build_model("smoke-llama", dtype=torch.bfloat16, seed=4),
                 w8_resident=True, **kw)
    assert res.w8_resident and res.use_graphs
    assert not L._FP8_REGISTRY and len(L._W8_RELEASED) == 9 + 10
    out_res = res.generate(list(PROMPT40), max_new_tokens=8)
    if chunk:
        assert res.stats["prefill_chunks"] == 3
    del res
    L._W8_RELEASED.clear()

    monkeypatch.setenv("RB_W8_PREFILL", "1")
    keep = Engine(build_model("smoke-llama", dtype=torch.bfloat16, seed=4),
                  **kw)
    assert not keep.w8_resident and keep.use_graphs
    assert len(L._FP8_REGISTRY) == 9 and not L._W8_RELEASED
    assert keep.model.lm_head.weight.is_cuda
    out_keep = keep.generate(list(PROMPT40), max_new_tokens=8)
    assert len(out_res) == 8
    assert out_res == out_keep, (out_res, out_keep)


def test_touching_a_released_master_raises():
    m = build_model("smoke-llama", dtype=torch.bfloat16, device=DEV, seed=5)
    fuse_for_inference(m, load_in_8bit=True, w8_resident=True)
    w = m.blocks[1].attn.o_proj.weight
    name = "blocks.1.attn.o_proj.weight"
    xb = torch.randn(4, w.shape[1], device=DEV).to(torch.bfloat16)
    bias = torch.zeros(w.shape[0], device=DEV, dtype=torch.bfloat16)
    with torch.no_grad():
        for args in ((xb.float(), w), (xb, w, bias)):
            with pytest.raises(RuntimeError, match=r"fp8-resident \(w8_res"
                               ) as ei:
                ops.fast_linear(*args)
            assert name in str(ei.value)
        # a per-projection view has no fp8 copy of its own
        with pytest.raises(RuntimeError, match="fp8-resident") as ei:
            ops.fast_linear(xb, m.blocks[0].attn.q_proj.weight)
        assert "q_proj.weight" in str(ei.value)
        assert ops.fast_linear(xb, w).shape == (4, w.shape[0])
        assert ops.decode_gemm_w8(xb, w).shape == (4, w.shape[0])
    with pytest.raises(RuntimeError, match=r"blocks\.0\.attn.*fp8-resident"):
        m.state_dict()
    with torch.enable_grad():
        with pytest.raises(RuntimeError, match=r"blocks\.0\..*fp8-resident"):
            m(torch.randint(0, 512, (1, 8), device=DEV))


def test_tied_embedding_keeps_its_master():
    eng = Engine(build_model("smoke-gemma", dtype=torch.bfloat16, seed=6),
                 device=DEV, kv_blocks=128, seed=1, load_in_8bit=True,
                 w8_resident=True)
    m = eng.model
    assert eng.w8_resident
    assert m.lm_head.weight is m.embed.weight and m.embed.weight.is_cuda
    assert L._w8_get(m.lm_head.weight) is not None   # decode streams fp8
    assert m.blocks[0].attn.o_proj.weight.device.type == "meta"
    out = eng.generate(list(PROMPT40), max_new_tokens=4)
    assert len(out) == 4 and all(0 <= t < m.cfg.vocab_size for t in out)
