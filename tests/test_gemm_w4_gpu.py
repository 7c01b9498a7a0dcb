"""int4 weight-only GEMM at any M (csrc/gemm_w4.hip) on the GPU: against
the exact dequant reference, row independence, ragged-tile padding, the
launcher's refusals and the fast_linear dispatch behind RB_W4_PREFILL."""
import functools

import pytest
import torch

from runbooks_amd import ops
from runbooks_amd.ops import linear as L

from test_w4_cpu import spread_weights

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _case(M, N, K):
    """-> (x bf16 [M,K] on GPU, wq_swz, sc_swz on GPU, y_ref f32 on CPU).
    Same construction as test_w4_gpu._case: per-group scales spread over
    [0.25, 4], the reference computed once on the CPU in fp32 from
    dequantize_int4(..., bf16), the kernel's exact weights. Cached: the
    tests below share it and leave it unchanged."""
    w = spread_weights(N, K, seed=M + N + K, outliers=False)
    q, s = L.quantize_int4(w)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(K + M)
                    ).to(torch.bfloat16)
    y_ref = x.float() @ L.dequantize_int4(q, s, torch.bfloat16).float().T
    wq_swz, sc_swz = ops.ext().w4_swizzle(q.to(DEV), s.to(DEV))
    return x.to(DEV), wq_swz, sc_swz, y_ref


# (M, N, K): the smallest shapes that exercise each way the kernel can go
# wrong (one m-tile template per M <= 32 / <= 64 / > 64, 128-row n-tiles)
SHAPES = [
    (33, 32, 64),        # one group, one n-block, one row past an m-tile
    (1, 64, 256),        # the M <= 32 edge the entry point still accepts
    (32, 64, 256),
    (64, 64, 256),       # an exact tile multiple
    (130, 96, 832),      # 13 groups, 3 n-blocks (ragged n-tile), ragged M
    (257, 512, 256),     # smoke qkv, many m-tiles plus 1
    (300, 256, 512),     # smoke down-proj
    (512, 4096, 4096),   # one real shape
]


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_kernel_matches_exact_dequant_reference(M, N, K):
    """max|y - y_ref| / max|y_ref| < 1e-2, the metric and bound of
    test_w4_gpu.test_kernel_matches_exact_dequant_reference: the weights
    are exact, so only the bf16 rounding of the output and the fp32
    summation order differ from the reference."""
    ext = ops.ext()
    assert ops.has_hip()
    assert ext.gemm_w4_supported(M, N, K)
    x, wq_swz, sc_swz, y_ref = _case(M, N, K)
    y = ext.gemm_w4(x, wq_swz, sc_swz, N, K)
    assert y.shape == (M, N) and y.dtype == torch.bfloat16
    err = (y.float().cpu() - y_ref).abs().max().item() / \
        y_ref.abs().max().item()
    print(f"gemm_w4 {M}x{N}x{K}: rel err {err:.3e}")
    assert err < 1e-2, err
    y2 = ext.gemm_w4(x, wq_swz, sc_swz, N, K)
    assert torch.equal(y, y2), "rerun not bitwise identical"


@pytest.mark.parametrize("r", [1, 33, 64, 129])
def test_row_independence(r):
    """gemm_w4(x)[:r] is bit-identical to gemm_w4(x[:r]): a row's sums do
    not depend on M, on its tile, or on the m-tile template M selects."""
    M, N, K = 130, 96, 832
    x, wq_swz, sc_swz, _ = _case(M, N, K)
    ext = ops.ext()
    full = ext.gemm_w4(x, wq_swz, sc_swz, N, K)
    part = ext.gemm_w4(x[:r].contiguous(), wq_swz, sc_swz, N, K)
    assert torch.equal(full[:r], part)


@pytest.mark.parametrize("M", [33, 130])
def test_padding_rows_are_never_read(M):
    """x is the first M rows of a larger buffer whose other rows are NaN:
    the ragged m-tile must not pull them in."""
    N, K = 96, 832
    x, wq_swz, sc_swz, _ = _case(130, N, K)
    big = torch.full((M + 128, K), float("nan"), dtype=torch.bfloat16,
                     device=DEV)
    big[:M] = x[:M]
    view = big[:M]
    assert view.is_contiguous() and view.data_ptr() == big.data_ptr()
    ext = ops.ext()
    y = ext.gemm_w4(view, wq_swz, sc_swz, N, K)
    assert torch.isfinite(y.float()).all()
    assert torch.equal(y, ext.gemm_w4(x[:M].clone(), wq_swz, sc_swz, N, K))


def test_launcher_refusals():
    ext = ops.ext()
    N, K = 64, 256
    x, wq_swz, sc_swz, _ = _case(32, N, K)
    assert ext.gemm_w4(x, wq_swz, sc_swz, N, K).shape == (32, N)
    with pytest.raises(RuntimeError, match="bf16"):
        ext.gemm_w4(x.float(), wq_swz, sc_swz, N, K)
    wide = torch.zeros(32, 2 * K, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="contiguous"):
        ext.gemm_w4(wide[:, :K], wq_swz, sc_swz, N, K)
    # K or N that do not match the swizzled tensors
    with pytest.raises(RuntimeError):
        ext.gemm_w4(wide, wq_swz, sc_swz, N, 2 * K)
    with pytest.raises(RuntimeError):
        ext.gemm_w4(x, wq_swz, sc_swz, 2 * N, K)
    with pytest.raises(RuntimeError):
        ext.gemm_w4(x[:, :128].contiguous(), wq_swz, sc_swz, N, K)
    with pytest.raises(RuntimeError):
        ext.gemm_w4(x, wq_swz, sc_swz[:1], N, K)
    # N % 32 != 0, K % 64 != 0
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ext.gemm_w4(x, wq_swz, sc_swz, 48, K)
    x96 = torch.zeros(32, 96, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ext.gemm_w4(x96, wq_swz, sc_swz, N, 96)
    # a CPU operand
    with pytest.raises(RuntimeError):
        ext.gemm_w4(x.cpu(), wq_swz, sc_swz, N, K)

    assert ext.gemm_w4_supported(1, 32, 64)
    assert ext.gemm_w4_supported(33, 64, 256)
    assert ext.gemm_w4_supported(2048, 12288, 4096)
    assert not ext.gemm_w4_supported(0, 64, 256)
    assert not ext.gemm_w4_supported(33, 48, 256)
    assert not ext.gemm_w4_supported(33, 64, 96)
    assert not ext.gemm_w4_supported(33, 0, 256)
    # 32-bit element offsets into x and y
    assert not ext.gemm_w4_supported(1 << 20, 4096, 64)
    assert not ext.gemm_w4_supported(1 << 20, 32, 4096)


def test_fast_linear_dispatch(monkeypatch):
    assert ops.has_hip()
    L._W4_REGISTRY.clear()
    try:
        N, K = 512, 256
        w = spread_weights(N, K, seed=9, outliers=False).to(
            torch.bfloat16).to(DEV)
        L.quantize_int4(w)
        q4 = L._registry_get(L._W4_REGISTRY, w)
        assert q4 is not None
        w2 = w.clone()                      # unregistered
        x33 = torch.randn(33, K, device=DEV).to(torch.bfloat16)
        x4 = torch.randn(4, K, device=DEV).to(torch.bfloat16)
        ext = ops.ext()
        with torch.no_grad():
            lin33 = torch.nn.functional.linear(x33, w)
            direct33 = ext.gemm_w4(x33, q4[0], q4[1], N, K)
            direct4 = ext.decode_gemm_w4(ext.decode_swizzle_x(x4), q4[0],
                                         q4[1], 4, N, K)
            assert not torch.equal(direct33, lin33)   # int4 rounding shows

            monkeypatch.setenv("RB_W4_PREFILL", "1")
            assert L.w4_prefill_enabled()
            assert torch.equal(ops.fast_linear(x33, w), direct33)
            # leading dimensions are flattened and restored
            y3 = ops.fast_linear(x33.view(3, 11, K), w)
            assert y3.shape == (3, 11, N)
            assert torch.equal(y3.view(33, N), direct33)
            assert torch.equal(ops.fast_linear(x4, w), direct4)
            assert torch.equal(ops.fast_linear(x33, w2),
                               torch.nn.functional.linear(x33, w2))

            monkeypatch.delenv("RB_W4_PREFILL")
            assert not L.w4_prefill_enabled()
            assert torch.equal(ops.fast_linear(x33, w), lin33)
            assert torch.equal(ops.fast_linear(x4, w), direct4)
            assert torch.equal(ops.fast_linear(x33, w2),
                               torch.nn.functional.linear(x33, w2))
    finally:
        L._W4_REGISTRY.clear()
