"""int4 weight-only decode path (MODEL_LOAD_IN_4BIT) on the GPU:
csrc/decode_gemm_w4.hip against its exact dequant reference, the
fast_linear dispatch, and the engine plumbing on smoke-llama."""
import pytest
import torch

from runbooks_amd import ops
from runbooks_amd.models import build_model
from runbooks_amd.ops import linear as L
from runbooks_amd.serve import Engine

from test_w4_cpu import spread_weights, w4_split_mirror, w4_swizzle_mirror

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _case(M, N, K):
    """-> (x bf16 [M,K] on GPU, canonical q, scales on GPU, y_ref f32).
    Weights carry per-group scales spread over [0.25, 4] so a mis-indexed
    scale cannot hide. The reference is computed on the CPU in fp32 from
    dequantize_int4(..., bf16), the kernel's exact weights."""
    w = spread_weights(N, K, seed=M + N + K, outliers=False)
    q, s = L.quantize_int4(w)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(K + M)
                    ).to(torch.bfloat16)
    y_ref = x.float() @ L.dequantize_int4(q, s, torch.bfloat16).float().T
    return x.to(DEV), q.to(DEV), s.to(DEV), y_ref


def _run(x, q, s, force_split=-1):
    ext = ops.ext()
    M, K = x.shape
    N = q.shape[0]
    wq_swz, sc_swz = ext.w4_swizzle(q, s)
    xs = ext.decode_swizzle_x(x)
    return ext.decode_gemm_w4(xs, wq_swz, sc_swz, M, N, K,
                              force_split=force_split)


# (M, N, K, force_split); -1 = the kernel's own choice
SHAPES = [
    (1, 32, 64, -1),        # one group, one block, three waves idle
    (5, 64, 256, -1),       # the smallest shape in smoke-llama
    (32, 512, 256, -1),     # smoke qkv
    (17, 256, 512, -1),     # smoke down-proj, odd M
    (32, 96, 832, -1),      # 13 groups: ring tail, uneven split, 3 n-blocks
    (32, 96, 832, 2),       # same through slabs + combine, one empty wave
    (32, 4096, 4096, -1),   # one real shape: the cross-WG split path
]


@pytest.mark.parametrize("M,N,K,force_split", SHAPES)
def test_kernel_matches_exact_dequant_reference(M, N, K, force_split):
    """max|y - y_ref| / max|y_ref| < 1e-2: the only legitimate difference
    is the bf16 rounding of the output (2^-9 relative) plus the fp32
    summation order; a CPU emulation of exactly that measured 1.8e-3 to
    2.9e-3 on these shape families, and a wrong scale or nibble lands
    orders of magnitude above the bound."""
    assert ops.has_hip()
    assert ops.ext().decode_gemm_w4_supported(M, N, K)
    if force_split < 0 and (N, K) == (4096, 4096):
        assert ops.ext().decode_gemm_w4_split(N, K) > 1
    x, q, s, y_ref = _case(M, N, K)
    y = _run(x, q, s, force_split)
    assert y.shape == (M, N) and y.dtype == torch.bfloat16
    err = (y.float().cpu() - y_ref).abs().max().item() / \
        y_ref.abs().max().item()
    print(f"w4 {M}x{N}x{K} split={force_split}: rel err {err:.3e}")
    assert err < 1e-2, err
    y2 = _run(x, q, s, force_split)
    assert torch.equal(y, y2), "rerun not bitwise identical"


def test_unsupported_shapes():
    ext = ops.ext()
    assert not ext.decode_gemm_w4_supported(33, 64, 256)
    assert not ext.decode_gemm_w4_supported(4, 48, 256)
    assert not ext.decode_gemm_w4_supported(4, 64, 96)
    for N, K in [(4096, 4096), (4096, 11008), (12288, 4096), (96, 832)]:
        assert ext.decode_gemm_w4_split(N, K) == w4_split_mirror(N, K)


@pytest.mark.parametrize("n,k", [(64, 256), (96, 832)])
def test_w4_swizzle_matches_python_mirror(n, k):
    q, s = L.quantize_int4(spread_weights(n, k, seed=n))
    wq_swz, sc_swz = ops.ext().w4_swizzle(q.to(DEV), s.to(DEV))
    m_wq, m_sc = w4_swizzle_mirror(q, s)
    assert wq_swz.shape == m_wq.shape and sc_swz.shape == m_sc.shape
    assert torch.equal(wq_swz.cpu(), m_wq)
    assert torch.equal(sc_swz.cpu().view(torch.int16), m_sc.view(torch.int16))


def test_fast_linear_dispatch():
    assert ops.has_hip()
    L._W4_REGISTRY.clear()
    try:
        N, K = 512, 256
        w = spread_weights(N, K, seed=9, outliers=False).to(
            torch.bfloat16).to(DEV)
        q, s = L.quantize_int4(w)
        assert q.is_cuda and L._registry_get(L._W4_REGISTRY, w) is not None
        deq = L.dequantize_int4(q, s, torch.bfloat16)

        x = torch.randn(4, K, device=DEV).to(torch.bfloat16)
        with torch.no_grad():
            y = ops.fast_linear(x, w)
            direct = _run(x, q, s)
            assert torch.equal(y, direct), "fast_linear did not run w4"
            ref = x.float() @ deq.float().T
            assert (y.float() - ref).abs().max().item() / \
                ref.abs().max().item() < 1e-2

            # producer-attached operand == swizzled here
            gamma = torch.ones(K, dtype=torch.bfloat16, device=DEV)
            xn, swz = ops.ext().rmsnorm_fwd_dec(x, gamma, 1e-5)
            y_plain = ops.fast_linear(xn, w)
            xn2 = xn.clone()
            xn2._rb_swz = swz
            y_swz = ops.fast_linear(xn2, w)
            assert torch.equal(y_plain, y_swz)

            # m = 33: F.linear on the bf16 master
            x33 = torch.randn(33, K, device=DEV).to(torch.bfloat16)
            assert torch.equal(ops.fast_linear(x33, w),
                               torch.nn.functional.linear(x33, w))

            # an unregistered weight is unaffected
            w2 = w.clone()
            assert L._registry_get(L._W4_REGISTRY, w2) is None
            assert torch.equal(ops.fast_linear(x, w2),
                               torch.nn.functional.linear(x, w2))
    finally:
        L._W4_REGISTRY.clear()


def test_paged_decode_operand_dh64():
    """Dh=64 (smoke-llama's head size): the int4 o_proj is the first
    consumer of the attention epilogue's fused operand at this width. The
    single-pass kernels emit it in 8-element units they do not have at
    Dh=64, so they must hand back NO operand; the split path's combine
    kernel emits one that equals decode_swizzle_x of the output."""
    assert ops.has_hip()
    torch.manual_seed(4)
    B, hkv, G, bs, nblk, dh = 3, 2, 2, 16, 16, 64
    kc = torch.randn(nblk, hkv, bs, dh, dtype=torch.bfloat16, device=DEV)
    vc = torch.randn_like(kc)
    q = torch.randn(B, hkv * G, dh, dtype=torch.bfloat16, device=DEV)
    bt = torch.arange(B * 4, dtype=torch.int32, device=DEV).reshape(B, 4)
    sl = torch.tensor([60, 33, 7], dtype=torch.int32, device=DEV)
    out1, swz1 = ops.paged_decode_with_operand(q, kc, vc, bt, sl, nsplit=1)
    assert swz1 is None
    out4, swz4 = ops.paged_decode_with_operand(q, kc, vc, bt, sl, nsplit=4)
    assert swz4 is not None
    K = hkv * G * dh
    ref = ops.ext().decode_swizzle_x(out4.reshape(B, K).contiguous())
    assert torch.equal(swz4.view(K // 16, 2, 32, 8)[:, :, :B],
                       ref.view(K // 16, 2, 32, 8)[:, :, :B])
    d = (out1.float() - out4.float()).abs().max() / out4.float().abs().max()
    assert d < 3e-2, d


def _w4_weights(model):
    out = []
    for blk in model.blocks:
        out += [blk.attn._qkv_w, blk.mlp._gateup_w, blk.attn.o_proj.weight,
                blk.mlp.down_proj.weight]
    return out + [model.lm_head.weight]


def test_engine_4bit_registers_and_generates():
    assert ops.has_hip()
    L._W4_REGISTRY.clear()
    try:
        m = build_model("smoke-llama", dtype=torch.bfloat16, seed=1)
        eng = Engine(m, device=DEV, kv_blocks=128, seed=3, load_in_4bit=True)
        ws = _w4_weights(eng.model)
        assert len(L._W4_REGISTRY) == len(ws) == 9
        for w in ws:
            assert L._registry_get(L._W4_REGISTRY, w) is not None
            assert L._registry_get(L._FP8_REGISTRY, w) is None
            assert L._registry_get(L._DECODE_W_REGISTRY, w) is None
        assert eng.use_graphs
        out = eng.generate([10, 20, 30], max_new_tokens=4)
        assert len(out) == 4 and all(0 <= t < m.cfg.vocab_size for t in out)

        # both knobs: 4-bit wins, nothing lands in the fp8 registry
        L._W4_REGISTRY.clear()
        both = Engine(build_model("smoke-llama", dtype=torch.bfloat16,
                                  seed=1),
                      device=DEV, kv_blocks=128, seed=3, load_in_4bit=True,
                      load_in_8bit=True)
        assert len(L._W4_REGISTRY) == 9
        for w in _w4_weights(both.model):
            assert L._registry_get(L._FP8_REGISTRY, w) is None
    finally:
        L._W4_REGISTRY.clear()


def test_engine_4bit_graph_matches_eager():
    assert ops.has_hip()
    L._W4_REGISTRY.clear()
    try:
        prompt = [5, 3, 8, 1, 9, 2]
        eng_g = Engine(build_model("smoke-llama", dtype=torch.bfloat16,
                                   seed=4),
                       device=DEV, kv_blocks=128, seed=11, load_in_4bit=True)
        assert eng_g.use_graphs
        out_g = eng_g.generate(list(prompt), max_new_tokens=8)
        eng_e = Engine(build_model("smoke-llama", dtype=torch.bfloat16,
                                   seed=4),
                       device=DEV, kv_blocks=128, seed=11, load_in_4bit=True)
        eng_e.use_graphs = False
        out_e = eng_e.generate(list(prompt), max_new_tokens=8)
        assert out_g == out_e, (out_g, out_e)
    finally:
        L._W4_REGISTRY.clear()


def test_4bit_decode_logits_match_fake_quantized_bf16():
    """Decode logits of a 4-bit model vs a bf16 model of the same seed
    whose weights went through fake_quantize_int4_, driven through
    model.prefill / model.decode like test_gemma_engine_decode_dh256
    (same metric, same 3e-2-of-max tolerance for a two-layer bf16 path
    comparison).

    Prefill always runs on the bf16 masters, so the 4-bit model's masters
    are fake-quantized too AFTER its int4 copies were taken from the
    original weights: both models then prefill identical weights, and the
    4-bit decode streams exactly the codes whose dequantization the
    reference holds in bf16."""
    from runbooks_amd.models.transformer import fuse_for_inference
    assert ops.has_hip()
    L._W4_REGISTRY.clear()
    try:
        prompt = [5, 9, 2, 7]
        m4 = build_model("smoke-llama", dtype=torch.bfloat16, device=DEV,
                         seed=11)
        fuse_for_inference(m4, load_in_4bit=True)
        ws4 = _w4_weights(m4)
        assert len(L._W4_REGISTRY) == len(ws4)
        for w in ws4:
            L.fake_quantize_int4_(w)           # in place: entries stay valid
            assert L._registry_get(L._W4_REGISTRY, w) is not None

        ref = build_model("smoke-llama", dtype=torch.bfloat16, device=DEV,
                          seed=11)
        fuse_for_inference(ref)
        for w in _w4_weights(ref):
            L.fake_quantize_int4_(w)
            assert L._registry_get(L._W4_REGISTRY, w) is None
            # a bf16 decode-layout copy taken before this edit would be stale
            assert L._registry_get(L._DECODE_W_REGISTRY, w) is None
        for a, b in zip(ws4, _w4_weights(ref)):
            assert torch.equal(a, b)

        S = len(prompt)

        def run(model):
            caches = model.alloc_caches(8, DEV)
            tokens = torch.tensor([prompt], dtype=torch.long, device=DEV)
            pos = torch.arange(S, dtype=torch.int32, device=DEV)
            slots = torch.arange(S, dtype=torch.int32, device=DEV)
            lp = model.prefill(tokens, pos, caches, slots)
            t = torch.tensor([3], dtype=torch.long, device=DEV)
            p = torch.tensor([S], dtype=torch.int32, device=DEV)
            sl = torch.tensor([S], dtype=torch.int32, device=DEV)
            bt = torch.tensor([[0, 1]], dtype=torch.int32, device=DEV)
            seq = torch.tensor([S + 1], dtype=torch.int32, device=DEV)
            ld = model.decode(t, p, caches, sl, bt, seq)
            return lp.float().cpu(), ld.float().cpu()

        with torch.no_grad():
            lp4, ld4 = run(m4)
            lpr, ldr = run(ref)
        for got, want in ((lp4, lpr), (ld4, ldr)):
            scale = want.abs().max().item()
            err = (got - want).abs().max().item() / scale
            print(f"w4 logits rel err {err:.3e}")
            assert err < 3e-2, (got[:, :8], want[:, :8])
    finally:
        L._W4_REGISTRY.clear()
