"""decode_gemm_mt.hip (bf16 weight-stream GEMM, 32 < M <= 256) on the GPU:
exact-arithmetic cases bit for bit, row identity with decode_gemm, an fp64
reference on random data, and the fast_linear dispatch behind
RB_DECODE_GEMM_MT."""
import functools

import pytest
import torch
import torch.nn.functional as F

from runbooks_amd import ops
from runbooks_amd.ops import linear as L

from test_decode_gemm_exact_cpu import exact_case_bf16

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

exact_case = functools.lru_cache(maxsize=None)(exact_case_bf16)


def ext():
    assert ops.has_hip(), "gfx950 extension not loaded"
    return ops.ext()


def _bits(y):
    return y.cpu().contiguous().view(torch.int16)


# (M, N, K, force_split): the smallest shapes that reach each edge
EXACT = [
    (33, 32, 1024, -1),     # one row into tile 2, one n-block, minimum K
    (64, 64, 1024, -1),     # exact tiles
    (65, 96, 1040, -1),     # ragged M; 65 k-steps: waves 17, 17, 17, 14
    (160, 64, 2048, -1),    # MT = 5, decode_gemm_split gives 2
    (256, 32, 4096, -1),    # MT = 8, decode_gemm_split gives 4
    (97, 64, 2048, 2),      # one ring pair per wave
    (97, 64, 2048, 4),      # tail-only waves
]


@pytest.mark.parametrize("M,N,K,fs", EXACT)
def test_exact_arithmetic(M, N, K, fs):
    """Inputs whose fp32 sums are exact in any order (the builder asserts
    it): y must be bf16_rne(exact sum) bit for bit."""
    e = ext()
    x, w, y_ref = exact_case(M, N, K, 0)
    if fs < 0 and M >= 160:
        assert e.decode_gemm_split(N, K) > 1
    y = e.decode_gemm_mt(x.to(DEV), e.decode_swizzle_w(w.to(DEV)), N, K,
                         force_split=fs)
    assert y.shape == (M, N) and y.dtype == torch.bfloat16
    assert torch.equal(_bits(y), _bits(y_ref))


@pytest.mark.parametrize("tag,N,heads", [("glu16", 64, (0, 0, 0)),
                                         ("rope16", 192, (1, 1, 64))])
def test_layout_tags_store_at_the_original_columns(tag, N, heads):
    e = ext()
    M, K = 65, 1040
    x, w, y_ref = exact_case(M, N, K, 0)
    x, w = x.to(DEV), w.to(DEV)
    plain = e.decode_gemm_mt(x, e.decode_swizzle_w(w), N, K)
    lid = L._LAYOUT_ID[tag]
    y = e.decode_gemm_mt(x, e.decode_swizzle_w_layout(w, lid, *heads), N, K,
                         lid, *heads)
    assert torch.equal(_bits(y), _bits(plain))
    assert torch.equal(_bits(y), _bits(y_ref))


@functools.lru_cache(maxsize=None)
def _random_case(M, N, K):
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV)
    w = torch.randn(N, K, generator=g).to(torch.bfloat16).to(DEV)
    return x, w, ext().decode_swizzle_w(w)


@pytest.mark.parametrize("M,N,K", [(160, 128, 4096), (70, 64, 1040)])
def test_row_identity_with_decode_gemm(M, N, K):
    """A row's sums depend on (N, K) alone: not on M, on the row's tile, or
    on which of the two kernels computes it."""
    e = ext()
    x, _, ws = _random_case(M, N, K)
    full = e.decode_gemm_mt(x, ws, N, K)
    for r0 in {0, 32, ((M - 1) // 32) * 32}:
        rows = x[r0:min(r0 + 32, M)].contiguous()
        y = e.decode_gemm(e.decode_swizzle_x(rows), ws, rows.shape[0], N, K)
        assert torch.equal(full[r0:r0 + rows.shape[0]], y), r0
    for r in (33, 64, 129):
        if r < M:
            part = e.decode_gemm_mt(x[:r].contiguous(), ws, N, K)
            assert torch.equal(full[:r], part), r


def test_fp64_reference_random():
    """max|y - y_ref| / max|y_ref| < 2e-2, the metric and bound of
    test_gpu_ops.test_decode_gemm."""
    M, N, K = 130, 96, 4096
    x, w, ws = _random_case(M, N, K)
    y = ext().decode_gemm_mt(x, ws, N, K)
    ref = x.cpu().double() @ w.cpu().double().t()
    rel = (y.cpu().double() - ref).abs().max().item() / ref.abs().max().item()
    print(f"decode_gemm_mt {M}x{N}x{K}: rel err {rel:.3e}")
    assert rel < 2e-2, rel


def test_dispatch_and_refusals(monkeypatch):
    e = ext()
    N, K = 64, 1024
    g = torch.Generator().manual_seed(4)
    w = torch.randn(N, K, generator=g).to(torch.bfloat16).to(DEV)
    w2 = w.clone()                          # unregistered
    bias = torch.zeros(N, dtype=torch.bfloat16, device=DEV)
    xs = {m: torch.randn(m, K, generator=g).to(torch.bfloat16).to(DEV)
          for m in (32, 40, 257)}
    L.register_decode_weight(w)
    try:
        ws = L._registry_get(L._DECODE_W_REGISTRY, w)[0]
        with torch.no_grad():
            direct = ops.decode_gemm_mt(xs[40], w)
            assert torch.equal(direct, e.decode_gemm_mt(xs[40], ws, N, K))
            with pytest.raises(RuntimeError, match="no registered"):
                ops.decode_gemm_mt(xs[40], w2)

            monkeypatch.setenv("RB_DECODE_GEMM_MT", "1")
            assert ops.decode_gemm_mt_enabled()
            assert torch.equal(ops.fast_linear(xs[40], w), direct)
            y3 = ops.fast_linear(xs[40].view(2, 20, K), w)
            assert y3.shape == (2, 20, N)
            assert torch.equal(y3.view(40, N), direct)
            assert torch.equal(ops.fast_linear(xs[257], w),
                               F.linear(xs[257], w))
            assert torch.equal(ops.fast_linear(xs[40], w, bias),
                               F.linear(xs[40], w, bias))
            assert torch.equal(ops.fast_linear(xs[40], w2),
                               F.linear(xs[40], w2))

            monkeypatch.delenv("RB_DECODE_GEMM_MT")
            assert not ops.decode_gemm_mt_enabled()
            assert torch.equal(ops.fast_linear(xs[40], w),
                               F.linear(xs[40], w))

        for m in (32, 257):
            assert not e.decode_gemm_mt_supported(m, N, K)
            with pytest.raises(RuntimeError, match="unsupported shape"):
                e.decode_gemm_mt(xs[m], ws, N, K)
        assert e.decode_gemm_mt_supported(33, N, K)
        assert e.decode_gemm_mt_supported(256, N, K)
        assert not e.decode_gemm_mt_supported(40, N, 1000)
        assert not e.decode_gemm_mt_supported(40, 48, K)
        x1000 = torch.zeros(40, 1000, dtype=torch.bfloat16, device=DEV)
        with pytest.raises(RuntimeError, match="unsupported shape"):
            e.decode_gemm_mt(x1000, ws, N, 1000)
        with pytest.raises(RuntimeError, match="ws size"):
            e.decode_gemm_mt(xs[40], ws[:-1], N, K)
        with pytest.raises(RuntimeError, match="bf16"):
            e.decode_gemm_mt(xs[40].float(), ws, N, K)
        with pytest.raises(RuntimeError, match="contiguous"):
            e.decode_gemm_mt(xs[40].t().contiguous().t(), ws, N, K)
        with pytest.raises(RuntimeError, match="layout"):
            e.decode_gemm_mt(xs[40], ws, N, K, 3)
    finally:
        L._DECODE_W_REGISTRY.clear()
