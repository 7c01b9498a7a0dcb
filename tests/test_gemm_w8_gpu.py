"""csrc/gemm_w8.hip, the fp8 weight-only GEMM at any M, in both forms."""
import functools

import pytest
import torch
import torch.nn.functional as F

from runbooks_amd import ops
from runbooks_amd.ops import linear as L

from test_decode_gemm_w8_gpu import E4M3, bits, exact_case, ref64

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def run(x, w8_swz, scale, form=-1):
    N = w8_swz.shape[0] * 32
    return ops.ext().gemm_w8(x, w8_swz, scale, N, x.shape[1], form)


@functools.lru_cache(maxsize=None)
def _random(M, N, K):
    """test_decode_gemm_w8_gpu.test_random's data; shared, never written."""
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w8 = (torch.randn(N, K, generator=g) * 64).to(E4M3).view(torch.uint8)
    scale = (0.25 + 3.75 * torch.rand(N, generator=g)) / 64
    return (x.to(DEV), ops.ext().w8_swizzle(w8.to(DEV)), scale.to(DEV),
            ref64(x, w8, scale))


# one group + one row into the second m-tile; MT = 1, two groups; exact tile
# multiple; MT = 4, 13 groups, ragged wide n-tile; second workgroup row
EXACT = [(33, 32, 64), (32, 64, 128), (64, 64, 256), (65, 96, 832),
         (130, 96, 832), (257, 160, 192)]


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("M,N,K", EXACT)
def test_exact(M, N, K, form):
    """Integer x in [-3, 3], codes in [-8, 8], power-of-two scales: partial
    sums <= 3*8*832 < 2^24, so y is bf16(fp64 reference) bit for bit; a
    permutation of k within or between a group's two blocks shows too."""
    x, w8, scale = exact_case(M, N, K)
    want = ref64(x, w8, scale).to(torch.bfloat16)
    got = run(x.to(DEV), ops.ext().w8_swizzle(w8.to(DEV)), scale.to(DEV),
              form).cpu()
    bad = (bits(got) != bits(want)).nonzero()
    assert len(bad) == 0, (len(bad), bad[:4].tolist())


@pytest.mark.parametrize("M,N,K", [(130, 96, 832), (512, 4096, 4096)])
def test_random(M, N, K):
    """One bf16 output rounding + fp32 order: the project's 1e-2 bound."""
    x, w8_swz, scale, ref = _random(M, N, K)
    y = run(x, w8_swz, scale)
    err = float((y.double().cpu() - ref).abs().max() / ref.abs().max())
    print(f"gemm_w8 {M}x{N}x{K}: rel err {err:.3e}")
    assert err < 1e-2
    assert torch.equal(bits(y), bits(run(x, w8_swz, scale)))


@pytest.mark.parametrize("r", [1, 33, 64, 129])
def test_row_independence(r):
    x, w8_swz, scale, _ = _random(130, 96, 832)
    full = run(x, w8_swz, scale)
    assert torch.equal(bits(full[:r]),
                       bits(run(x[:r].contiguous(), w8_swz, scale)))


@pytest.mark.parametrize("M", [33, 130])
def test_forms_equal_and_padding_rows_never_read(M):
    """x is the first M rows of a NaN-filled buffer; wide == narrow."""
    x, w8_swz, scale, _ = _random(130, 96, 832)
    big = torch.full((M + 128, 832), float("nan"), dtype=torch.bfloat16,
                     device=DEV)
    big[:M] = x[:M]
    want = run(x[:M].clone(), w8_swz, scale, 0)
    for form in (0, 1):
        y = run(big[:M], w8_swz, scale, form)
        assert torch.isfinite(y.float()).all()
        assert torch.equal(bits(y), bits(want))


def test_launcher_refusals():
    e = ops.ext()
    N, K = 64, 128
    x, w8, scale = exact_case(32, N, K)
    x, w8_swz, scale = x.to(DEV), e.w8_swizzle(w8.to(DEV)), scale.to(DEV)
    assert e.gemm_w8(x, w8_swz, scale, N, K).shape == (32, N)
    wide = torch.zeros(32, 2 * K, dtype=torch.bfloat16, device=DEV)
    x96 = torch.zeros(32, 96, dtype=torch.bfloat16, device=DEV)
    for args, match in (
            ((x.float(), w8_swz, scale, N, K), "bf16"),
            ((x, w8_swz, scale.double(), N, K), "f32"),
            ((wide[:, :K], w8_swz, scale, N, K), "contiguous"),
            ((wide, w8_swz, scale, N, 2 * K), "w8_swz holds"),
            ((x, w8_swz, scale, 2 * N, K), "w8_swz holds"),
            ((x[:, :64].contiguous(), w8_swz, scale, N, K), "K ="),
            ((x, w8_swz, scale[:32], N, K), "scale holds"),
            ((x, w8_swz, scale, 48, K), "unsupported shape"),
            ((x96, w8_swz, scale, N, 96), "unsupported shape"),
            ((x.cpu(), w8_swz, scale, N, K), "one GPU"),
            ((x, w8_swz, scale, N, K, 2), "form")):
        with pytest.raises(RuntimeError, match=match):
            e.gemm_w8(*args)
    for shape, ok in (((1, 32, 64), True), ((2048, 12288, 4096), True),
                      ((0, 64, 128), False), ((33, 48, 128), False),
                      ((33, 64, 96), False), ((33, 0, 128), False),
                      # 32-bit element offsets into y and x
                      ((1 << 20, 4096, 64), False),
                      ((1 << 20, 32, 4096), False)):
        assert e.gemm_w8_supported(*shape) == ok, shape


def test_fast_linear_dispatch(monkeypatch):
    e = ops.ext()
    monkeypatch.setenv("RB_DECODE_GEMM_W8", "1")
    monkeypatch.delenv("RB_W8_PREFILL", raising=False)
    L._FP8_REGISTRY.clear()
    try:
        g = torch.Generator().manual_seed(7)
        N, K = 256, 512
        w = torch.randn(N, K, generator=g).to(torch.bfloat16).to(DEV)
        w2 = w.clone()                      # unregistered
        x33 = torch.randn(33, K, generator=g).to(torch.bfloat16).to(DEV)
        x4 = x33[:4].contiguous()
        L.quantize_fp8(w)
        q = L._registry_get(L._FP8_REGISTRY, w)
        with torch.no_grad():
            direct33 = e.gemm_w8(x33, q[0], q[1], N, K)
            direct4 = e.decode_gemm_w8(e.decode_swizzle_x(x4), q[0], q[1],
                                       4, N, K)
            lin33 = F.linear(x33, w)
            assert not torch.equal(direct33, lin33)    # fp8 rounding shows
            assert torch.equal(bits(ops.fast_linear(x33, w)), bits(lin33))

            monkeypatch.setenv("RB_W8_PREFILL", "1")
            assert torch.equal(bits(ops.fast_linear(x33, w)), bits(direct33))
            assert torch.equal(bits(ops.gemm_w8(x33, w)), bits(direct33))
            y3 = ops.fast_linear(x33.view(3, 11, K), w)
            assert y3.shape == (3, 11, N)
            assert torch.equal(bits(y3.view(33, N)), bits(direct33))
            assert torch.equal(bits(ops.fast_linear(x4, w)), bits(direct4))
            assert torch.equal(bits(ops.fast_linear(x33, w2)),
                               bits(F.linear(x33, w2)))
    finally:
        L._FP8_REGISTRY.clear()
