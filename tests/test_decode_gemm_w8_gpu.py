"""csrc/decode_gemm_w8.hip, the fp8 weight-stream decode GEMM
(MODEL_LOAD_IN_8BIT, M <= 32): exact arithmetic and needles at tolerance
zero, random data against an fp64 reference, the fast_linear dispatch and
the engine on smoke-llama.

Partitions the exact cases reach, U = 4: main + tail blocks (of 32 k) per
wave; main blocks run through the 2U = 8 block ring, tail blocks as one or
two clamped chunks. split -1 is decode_gemm_w8_split's choice at N <= 96.

  K=32    split=1 (-1)   1 block:  0+1, empty x3
  K=32    split=2        0+1, empty x7
  K=32    split=8        0+1, empty x31
  K=1024  split=1 (-1)  32 blocks: 8+0 x4           one pair, tail 0
  K=1024  split=2        0+4 x8
  K=1024  split=8        0+1 x32
  K=1056  split=1 (-1)  33 blocks: 8+1 x3, 0+6      tail-only wave, 2 chunks
  K=1056  split=2        0+5 x6, 0+3, empty          empty wave
  K=1056  split=8        0+2 x16, 0+1, empty x15     empty k-slices 5..7
  K=1152  split=1 (-1)  36 blocks: 8+1 x4           tail 1
  K=1152  split=2        0+5 x7, 0+1
  K=1152  split=8        0+2 x18, empty x14
  K=1920  split=1 (-1)  60 blocks: 8+7 x4           tail 2U-1
  K=1920  split=2        8+0 x7, 0+4
  K=1920  split=8        0+2 x30, empty x2
  K=4096  split=4 (-1) 128 blocks: 8+0 x16
  K=4096  split=2        16+0 x8                     two pairs
  K=4096  split=8        0+4 x32
  K=6400  split=4 (-1) 200 blocks: 8+5 x15, 0+5
  K=6400  split=2        24+1 x8                     three pairs, tail 1
  K=6400  split=8        0+7 x28, 0+4, empty x3
"""
import pytest
import torch
import torch.nn.functional as F

from runbooks_amd import ops
from runbooks_amd.models import build_model
from runbooks_amd.ops import linear as L
from runbooks_amd.serve import Engine

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
E4M3 = torch.float8_e4m3fn


def run(x, w8, scale, split=-1, tail=-1):
    """x [M,K] bf16, canonical e4m3 bytes [N,K], f32 scale [N] (CPU) -> y."""
    e = ops.ext()
    (M, K), N = x.shape, w8.shape[0]
    return e.decode_gemm_w8(e.decode_swizzle_x(x.to(DEV)),
                            e.w8_swizzle(w8.to(DEV)), scale.to(DEV),
                            M, N, K, split, tail).cpu()


def ref64(x, w8, scale):
    return x.double() @ w8.view(E4M3).double().T * scale.double()


def bits(t):
    return t.contiguous().view(torch.int16)


def exact_case(M, N, K):
    g = torch.Generator().manual_seed(1000 * M + N + K)
    x = torch.randint(-3, 4, (M, K), generator=g).to(torch.bfloat16)
    w8 = torch.randint(-8, 9, (N, K), generator=g).float().to(E4M3)
    scale = 2.0 ** torch.randint(-3, 4, (N,), generator=g).float()
    return x, w8.view(torch.uint8), scale


@pytest.mark.parametrize("split", [-1, 2, 8])
@pytest.mark.parametrize("K", [32, 1024, 1056, 1152, 1920, 4096, 6400])
def test_exact(K, split):
    """Integer x in [-3, 3], integer codes in [-8, 8], power-of-two scales:
    every partial sum is an integer below 2^24, so the fp32 sum is exact in
    any order and y is bf16(fp64 reference) bit for bit."""
    for M in (1, 17, 32):
        for N in (32, 96):
            x, w8, scale = exact_case(M, N, K)
            want = ref64(x, w8, scale).to(torch.bfloat16)
            got = run(x, w8, scale, split)
            bad = (bits(got) != bits(want)).nonzero()
            assert len(bad) == 0, (M, N, K, split, len(bad), bad[:4].tolist())


@pytest.mark.parametrize("K,split", [(1056, 1), (6400, 2)])
def test_ring_tail_equals_tail_loop(K, split):
    x, w8, scale = exact_case(17, 96, K)
    assert torch.equal(bits(run(x, w8, scale, split, tail=0)),
                       bits(run(x, w8, scale, split, tail=1)))


@pytest.mark.parametrize("launch", range(8))
def test_needle_every_code(launch):
    """x row m = e_k, k = 32 * launch + m, so y[m, n] is scale[n] *
    value(W8[n, k]) with nothing else in the sum. Row n of W8 walks all 254
    finite codes, subnormals and -0 included; the scales carry 6
    significant bits, so scale * value is exact in fp32 and rounds once.
    K = 256 at split 1 is 0+2 blocks per wave: over the eight launches
    every k of every wave range and tail chunk is probed. The zero products
    of the other k make the sum +0 where the code is -0, so zeros compare
    by value (y + 0.0), everything else by bits."""
    N, K = 32, 256
    codes = torch.tensor([c for c in range(256) if c & 0x7F != 0x7F],
                         dtype=torch.uint8)
    idx = (torch.arange(K)[None, :] + 8 * torch.arange(N)[:, None]) % 254
    w8 = codes[idx]
    scale = (1 + torch.arange(N) / 32.0) * 2.0 ** (torch.arange(N) % 5 - 2)
    ks = 32 * launch + torch.arange(32)
    x = torch.zeros(32, K, dtype=torch.bfloat16)
    x[torch.arange(32), ks] = 1
    want = (scale.double()[None, :] *
            w8.view(E4M3).double().T[ks]).to(torch.bfloat16)
    got = run(x, w8, scale)
    bad = (bits(got + 0.0) != bits(want + 0.0)).nonzero()
    assert len(bad) == 0, [(int(ks[m]), n, int(w8[n, ks[m]]),
                            float(got[m, n]), float(want[m, n]))
                           for m, n in bad[:6].tolist()]


@pytest.mark.parametrize("M,N,K", [(5, 64, 256), (17, 256, 512),
                                   (32, 4096, 4096)])
def test_random(M, N, K):
    """max|y - ref| / max|ref| < 1e-2 against fp64: one bf16 output
    rounding (2^-9) plus the fp32 summation order, the bound and rationale
    of tests/test_w4_gpu.py. Per-row scales spread over [0.25, 4]."""
    if N == 4096:
        assert ops.ext().decode_gemm_w8_split(N, K) > 1
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w8 = (torch.randn(N, K, generator=g) * 64).to(E4M3).view(torch.uint8)
    scale = (0.25 + 3.75 * torch.rand(N, generator=g)) / 64
    ref = ref64(x, w8, scale)
    y = run(x, w8, scale)
    err = float((y.double() - ref).abs().max() / ref.abs().max())
    print(f"decode_gemm_w8 {M}x{N}x{K}: rel err {err:.3e}")
    assert err < 1e-2
    assert torch.equal(bits(y), bits(run(x, w8, scale)))


def test_dispatch(monkeypatch):
    e = ops.ext()
    for shape in ((33, 64, 64), (1, 48, 64), (1, 64, 48)):
        assert not e.decode_gemm_w8_supported(*shape)
    g = torch.Generator().manual_seed(7)
    N, K = 256, 512
    w = torch.randn(N, K, generator=g).to(torch.bfloat16).to(DEV)
    x = torch.randn(17, K, generator=g).to(torch.bfloat16).to(DEV)
    L._FP8_REGISTRY.clear()
    try:
        with torch.no_grad():
            with pytest.raises(RuntimeError, match="registration"):
                ops.decode_gemm_w8(x, w)
            monkeypatch.setenv("RB_DECODE_GEMM_W8", "1")
            w8, scale = L.quantize_fp8(w)
            q = L._registry_get(L._FP8_REGISTRY, w)
            assert q[2] == (N, K) and q[0].shape == (N // 32, K // 32, 64, 16)
            direct = e.decode_gemm_w8(e.decode_swizzle_x(x), e.w8_swizzle(w8),
                                      scale, 17, N, K)
            assert torch.equal(bits(L.fast_linear(x, w)), bits(direct))
            assert torch.equal(bits(ops.decode_gemm_w8(x, w)), bits(direct))
            # a producer-attached operand: same rows, same bits
            h = torch.randn(17, K, generator=g).to(torch.bfloat16).to(DEV)
            xn = ops.rmsnorm(h, torch.ones(K, dtype=torch.bfloat16,
                                           device=DEV))
            assert getattr(xn, "_rb_swz", None) is not None
            assert torch.equal(bits(L.fast_linear(xn, w)),
                               bits(L.fast_linear(xn.clone(), w)))
            x33 = torch.randn(33, K, generator=g).to(torch.bfloat16).to(DEV)
            assert torch.equal(bits(L.fast_linear(x33, w)),
                               bits(F.linear(x33, w)))
            # the old path, chosen at quantize time
            monkeypatch.setenv("RB_DECODE_GEMM_W8", "0")
            w8, scale = L.quantize_fp8(w)
            assert L._registry_get(L._FP8_REGISTRY, w)[2] is None
            assert torch.equal(bits(L.fast_linear(x, w)),
                               bits(e.skinny_gemm_fp8(x, w8, scale)))
    finally:
        L._FP8_REGISTRY.clear()


def test_engine_8bit(monkeypatch):
    monkeypatch.setenv("RB_DECODE_GEMM_W8", "1")
    L._FP8_REGISTRY.clear()
    try:
        outs = []
        for graphs in (True, False):
            eng = Engine(build_model("smoke-llama", dtype=torch.bfloat16,
                                     seed=4),
                         device=DEV, kv_blocks=128, seed=11, load_in_8bit=True)
            ws = [eng.model.lm_head.weight]
            for blk in eng.model.blocks:
                ws += [blk.attn._qkv_w, blk.mlp._gateup_w,
                       blk.attn.o_proj.weight, blk.mlp.down_proj.weight]
            assert len(ws) == 9
            for w in ws:
                assert L._registry_get(L._FP8_REGISTRY, w)[2] == \
                    tuple(w.shape)
            assert eng.use_graphs
            eng.use_graphs = graphs
            outs.append(eng.generate([5, 3, 8, 1, 9, 2], max_new_tokens=8))
        assert outs[0] == outs[1], outs
    finally:
        L._FP8_REGISTRY.clear()
