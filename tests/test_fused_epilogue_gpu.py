"""Fused decode-GEMM epilogues (csrc/decode_gemm.hip) on the GPU: the
un-permuting store on glu16 / rope16 weight layouts, the SwiGLU / GeGLU
epilogue, the RoPE + KV-append epilogue, and the model-level switch
RB_FUSED_EPILOGUE.

Every check is torch.equal against today's kernel sequence on a
plain-layout weight: a row permutation leaves each sum's k-order and the
4-wave reduce order alone, the sums are rounded to bf16 at the same point,
and the activation / RoPE expressions are the shared helpers of common.h.
"""
import os

import pytest
import torch

from runbooks_amd import ops
from runbooks_amd.models import build_model
from runbooks_amd.models.config import ModelConfig
from runbooks_amd.models.transformer import fuse_for_inference
from runbooks_amd.ops import linear as L
from runbooks_amd.serve import Engine

from test_fused_epilogue_cpu import glu16_perm, rope16_perm

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K = 1024                     # smallest decode_gemm_supported K
MS = [1, 5, 32]
BS = ops.BLOCK_SIZE


def _randn(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).to(DEV)


@pytest.fixture(autouse=True)
def _clean_registry():
    assert ops.has_hip()
    L._DECODE_W_REGISTRY.clear()
    yield
    L._DECODE_W_REGISTRY.clear()


def _operand_rows(swz, m):
    """rows < m of a decode operand [K/16][hi][32][8]"""
    return swz.view(-1, 2, 32, 8)[:, :, :m]


# ---- layouts ----------------------------------------------------------------
def test_layout_swizzle_is_swizzle_of_permuted_rows():
    ext = ops.ext()
    w = _randn(2 * 48, 64, seed=1)
    perm = torch.from_numpy(glu16_perm(48)).to(DEV)
    assert torch.equal(ext.decode_swizzle_w_layout(w, 1),
                       ext.decode_swizzle_w(w[perm].contiguous()))
    hq, hkv, dh = 2, 1, 64
    w = _randn((hq + 2 * hkv) * dh, 64, seed=2)
    perm = torch.from_numpy(rope16_perm(hq, hkv, dh)).to(DEV)
    assert torch.equal(ext.decode_swizzle_w_layout(w, 2, hq, hkv, dh),
                       ext.decode_swizzle_w(w[perm].contiguous()))
    assert torch.equal(ext.decode_swizzle_w_layout(w, 0),
                       ext.decode_swizzle_w(w))


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("layout", ["glu16", "rope16"])
def test_unpermuting_store_equals_plain_layout(M, layout):
    hq, hkv, dh = 8, 2, 128
    n = 2 * 1040 if layout == "glu16" else (hq + 2 * hkv) * dh
    w = _randn(n, K, seed=n, scale=0.05)
    x = _randn(M, K, seed=M)
    with torch.no_grad():
        L.register_decode_weight(w)
        assert L.decode_layout(w) == "plain"
        y_plain = ops.fast_linear(x, w)
        raw_plain, _ = ops.decode_linear_raw(x, w)
        L.register_decode_weight(w, layout, hq, hkv, dh)
        assert L.decode_layout(w) == layout
        y = ops.fast_linear(x, w)
        raw, slab = ops.decode_linear_raw(x, w)
    assert not slab
    assert torch.equal(y, y_plain)
    assert torch.equal(raw, raw_plain)
    # and it is the product, not merely self-consistent
    ref = x.float() @ w.float().t()
    assert (y.float() - ref).abs().max() / ref.abs().max() < 2e-2


def test_unpermuting_store_through_split_k_slabs():
    """force_split: the fp32 slab store un-permutes the same way."""
    ext = ops.ext()
    hq, hkv, dh = 2, 2, 64
    n = (hq + 2 * hkv) * dh
    w = _randn(n, 2048, seed=9, scale=0.05)
    xs = ext.decode_swizzle_x(_randn(5, 2048, seed=10))
    y_plain = ext.decode_gemm(xs, ext.decode_swizzle_w(w), 5, n, 2048, 2)
    y = ext.decode_gemm(xs, ext.decode_swizzle_w_layout(w, 2, hq, hkv, dh),
                        5, n, 2048, 2, 2, hq, hkv, dh)
    assert torch.equal(y, y_plain)


# ---- GLU epilogue -----------------------------------------------------------
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("inter", [1040, 16])
@pytest.mark.parametrize("gelu", [False, True], ids=["swiglu", "geglu"])
def test_glu_epilogue_equals_packed_kernel(M, inter, gelu):
    ext = ops.ext()
    w = _randn(2 * inter, K, seed=inter, scale=0.05)
    x = _randn(M, K, seed=M + 7)
    xs = ext.decode_swizzle_x(x)
    y = ext.decode_gemm(xs, ext.decode_swizzle_w(w), M, 2 * inter, K)
    h_ref, swz_ref = (ext.geglu_packed_dec if gelu
                      else ext.swiglu_packed_dec)(y)
    assert h_ref.float().abs().max() > 0

    L.register_decode_weight(w, "glu16")
    assert ops.fused_epilogue_ok(x, w, "glu16")
    swz, m = ops.decode_linear_glu(x, w, gelu=gelu)
    assert m == M and swz.shape == swz_ref.shape
    assert torch.equal(_operand_rows(swz, M), _operand_rows(swz_ref, M))

    if inter >= 1024:       # a down-proj the decode GEMM supports (K = I)
        wd = _randn(256, inter, seed=3, scale=0.05)
        L.register_decode_weight(wd)
        h_ref._rb_swz = swz_ref
        out_ref, _ = ops.decode_linear_raw(h_ref, wd)
        out, _ = ops.decode_linear_raw(None, wd, xs=swz, m=M)
        assert torch.equal(out, out_ref)


# ---- RoPE + append epilogue -------------------------------------------------
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("hq,hkv,dh", [(8, 8, 128), (8, 2, 128), (4, 4, 64),
                                       (2, 2, 256)])
def test_rope_append_epilogue_equals_separate_kernel(M, hq, hkv, dh):
    ext = ops.ext()
    n = (hq + 2 * hkv) * dh
    w = _randn(n, K, seed=n + dh, scale=0.05)
    x = _randn(M, K, seed=M + 11)
    cos, sin = ops.rope_tables(dh, 64, 10000.0)
    cos, sin = cos.to(DEV), sin.to(DEV)
    # non-monotonic positions; slots over blocks 1 and 2, one row skipped
    pos = torch.tensor([(37 * i + 5) % 61 for i in range(M)],
                       dtype=torch.int32, device=DEV)
    slot_list = [BS + (i * 7) % (2 * BS) for i in range(M)]
    assert len(set(slot_list)) == M              # 7 is coprime to 32
    if M > 1:
        slot_list[M // 2] = -1
    else:
        slot_list[0] = 2 * BS + 3
    slots = torch.tensor(slot_list, dtype=torch.int32, device=DEV)

    vt = hq // hkv >= 4 and dh <= 128            # Transformer.alloc_caches
    kc0, vc0 = ops.alloc_kv_cache(4, hkv, dh, DEV, v_transposed=vt)
    kc0.copy_(_randn(*kc0.shape, seed=1))        # sentinel contents
    vc0.copy_(_randn(*vc0.shape, seed=2))
    assert (vc0.shape[2] == dh and dh != BS) == vt

    xs = ext.decode_swizzle_x(x)
    y = ext.decode_gemm(xs, ext.decode_swizzle_w(w), M, n, K)
    kc_ref, vc_ref = kc0.clone(), vc0.clone()
    q_ref = ext.qkv_rope_append(y, cos, sin, pos, kc_ref, vc_ref, slots, hq)

    L.register_decode_weight(w, "rope16", hq, hkv, dh)
    assert ops.fused_epilogue_ok(x, w, "rope16")
    kc, vc = kc0.clone(), vc0.clone()
    q = ops.decode_linear_rope_append(x, w, cos, sin, pos, kc, vc, slots, hq)
    assert q.shape == (M, hq, dh)
    assert torch.equal(q, q_ref)
    assert torch.equal(kc, kc_ref)
    assert torch.equal(vc, vc_ref)

    # entries outside the written slots are unchanged
    written = torch.zeros(4 * BS, dtype=torch.bool, device=DEV)
    written[[s for s in slot_list if s >= 0]] = True
    keep = ~written.view(4, 1, BS, 1)
    assert torch.equal(kc[keep.expand_as(kc)], kc0[keep.expand_as(kc0)])
    keep_v = keep.transpose(2, 3) if vt else keep
    assert torch.equal(vc[keep_v.expand_as(vc)], vc0[keep_v.expand_as(vc0)])
    # and the written ones did change
    assert not torch.equal(kc, kc0) and not torch.equal(vc, vc0)


def _fma_f32(x, y, z):
    """fma(x, y, z) of f32 tensors, rounded once. x*y is exact in f64
    (24 + 24 bits); the f64 sum is rounded to odd (TwoSum gives its exact
    error), so the final rounding to f32 is the single rounding of the
    exact value, as in a hardware fma."""
    p = x.double() * y.double()
    z = z.double().expand_as(p)
    t = p + z
    zz = t - p
    err = (p - (t - zz)) + (z - zz)
    ti = t.contiguous().view(torch.int64)
    away = torch.where((err > 0) == (t > 0), 1, -1)
    fix = (err != 0) & ((ti & 1) == 0)
    return torch.where(fix, ti + away, ti).view(torch.float64).float()


def test_shared_rope_helper_keeps_the_standalone_kernels_rounding():
    """rope_rot (common.h) pins which product is rounded on its own:
    o1 = fma(a, c, -(b*s)), o2 = fma(a, s, b*c) — what the standalone
    kernel computed before the expression was shared. The fused-vs-separate
    checks above cannot see a change made to both at once; this one compares
    the separate kernel against an exactly rounded fma built in float64.

    The two contractions differ by an f32 ulp in a fair share of the
    elements, but a bf16 output flips only when that ulp straddles a bf16
    rounding boundary (about 2^-16 of them), so the check needs millions
    of elements to tell them apart: T = 4096 rows of 32 heads, q only
    (every slot is -1, nothing is appended)."""
    ext = ops.ext()
    T, hq, hkv, dh = 4096, 32, 1, 128
    half = dh // 2
    y = _randn(T, (hq + 2 * hkv) * dh, seed=21)
    cos, sin = ops.rope_tables(dh, T, 10000.0)
    cos, sin = cos.to(DEV), sin.to(DEV)
    pos = torch.arange(T, dtype=torch.int32, device=DEV)
    slots = torch.full((T,), -1, dtype=torch.int32, device=DEV)
    kc, vc = ops.alloc_kv_cache(1, hkv, dh, DEV)
    q = ext.qkv_rope_append(y, cos, sin, pos, kc, vc, slots, hq)

    yq = y[:, :hq * dh].view(T, hq, dh).float()
    a, b = yq[..., :half], yq[..., half:]
    c = cos.view(T, 1, half)
    s = sin.view(T, 1, half)

    fma = _fma_f32

    o1 = fma(a, c, -(b * s))
    o2 = fma(a, s, b * c)
    ref = torch.cat([o1, o2], -1).to(torch.bfloat16)
    assert torch.equal(q, ref)
    # the data tells the two contractions of o2 apart
    other = torch.cat([o1, fma(b, c, a * s)], -1).to(torch.bfloat16)
    assert not torch.equal(other, ref)


# ---- model level ------------------------------------------------------------
def _cfg(hkv):
    return ModelConfig(f"fused-epi-test-kv{hkv}", vocab_size=512,
                       hidden_size=1024, num_layers=2, num_heads=8,
                       num_kv_heads=hkv, intermediate_size=1040,
                       max_seq_len=256)


class _env:
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("RB_FUSED_EPILOGUE")
        os.environ["RB_FUSED_EPILOGUE"] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            del os.environ["RB_FUSED_EPILOGUE"]
        else:
            os.environ["RB_FUSED_EPILOGUE"] = self.old


def _prefill_and_decode(model, B=3, S=6, steps=3):
    caches = model.alloc_caches(2 * B + 1, DEV)
    g = torch.Generator().manual_seed(5)
    tokens = torch.randint(0, 512, (B, S), generator=g).to(DEV)
    pos = torch.arange(S, dtype=torch.int32, device=DEV).repeat(B)
    # sequence b owns blocks 2b, 2b+1
    slots = torch.cat([torch.arange(S, dtype=torch.int32) + 2 * b * BS
                       for b in range(B)]).to(DEV)
    bt = torch.tensor([[2 * b, 2 * b + 1] for b in range(B)],
                      dtype=torch.int32, device=DEV)
    out = [model.prefill(tokens, pos, caches, slots)]
    for i in range(steps):
        t = out[-1].argmax(-1)
        p = torch.full((B,), S + i, dtype=torch.int32, device=DEV)
        sl = torch.tensor([2 * b * BS + S + i for b in range(B)],
                          dtype=torch.int32, device=DEV)
        seq = torch.full((B,), S + i + 1, dtype=torch.int32, device=DEV)
        out.append(model.decode(t, p, caches, sl, bt, seq))
    return torch.stack(out), caches


@pytest.mark.parametrize("hkv", [8, 2])
def test_model_logits_equal_with_and_without_fused_epilogue(hkv):
    model = build_model(_cfg(hkv), dtype=torch.bfloat16, device=DEV, seed=3)
    fuse_for_inference(model)
    blk = model.blocks[0]
    assert L.decode_layout(blk.attn._qkv_w) == "rope16"
    assert L.decode_layout(blk.mlp._gateup_w) == "glu16"
    assert L.decode_layout(blk.mlp.down_proj.weight) == "plain"
    assert L.decode_layout(model.lm_head.weight) == "plain"
    x = torch.zeros(3, 1024, dtype=torch.bfloat16, device=DEV)
    with _env("1"):
        assert ops.fused_epilogue_ok(x, blk.attn._qkv_w, "rope16")
        assert ops.fused_epilogue_ok(x, blk.mlp._gateup_w, "glu16")
        fused, caches_f = _prefill_and_decode(model)
    with _env("0"):
        assert not ops.fused_epilogue_ok(x, blk.attn._qkv_w, "rope16")
        plain, caches_p = _prefill_and_decode(model)
    assert torch.equal(fused, plain)
    for (kf, vf), (kp, vp) in zip(caches_f, caches_p):
        assert torch.equal(kf, kp) and torch.equal(vf, vp)


def test_engine_graph_tokens_equal_with_and_without_fused_epilogue():
    prompt = [5, 3, 8, 1, 9, 2]
    outs = []
    for flag in ("1", "0"):
        with _env(flag):
            eng = Engine(build_model(_cfg(2), dtype=torch.bfloat16, seed=4),
                         device=DEV, kv_blocks=64, seed=11)
            assert eng.use_graphs
            outs.append(eng.generate(list(prompt), max_new_tokens=6))
    assert outs[0] == outs[1], outs
