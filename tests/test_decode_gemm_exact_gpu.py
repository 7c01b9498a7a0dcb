"""The weight-stream GEMMs against exact arithmetic, tolerance zero.

decode_gemm.hip, decode_gemm_w4.hip and gemm_w4.hip accumulate bf16 x bf16
products in fp32. The cases come from test_decode_gemm_exact_cpu.py: every
product and partial sum of an output is a multiple of one power of two
below 2^24 of them, so the fp32 sum is exact in any order and the output
must be bf16_rne(exact sum) bit for bit, whatever the ring depth, k-split
or reduce tree. That module proves on a CPU mirror of the kernels that one
lost, doubled or misplaced k-step, lane fragment, nibble or scale changes
at least one output bit of every case used here, so a kernel with such a
fault fails this module. Needle cases (x row m = e_ks[m], so y[m, n] is
w[n, ks[m]]) probe the first and last k of every wave range, ring half and
tail, and name the k that was lost.

Partitions reached, per kernel: main + tail units per wave (a unit is a
k-step of 16 for decode_gemm, a group of 64 k for decode_gemm_w4; main
units run through the 2U ring, tail units one by one). Printed by
test_decode_gemm_exact_cpu.print_partition_table(); its
test_case_lists_reach_every_edge asserts tail 0, 1 and 2U-1, a tail-only
wave, an empty wave, an empty k-slice and 1, 2 and 3 ring pairs for each.

decode_gemm U=8
  K=1024  split=1   64 units: 16+0 x4
  K=1024  split=2   64 units: 0+8 x8
  K=1040  split=1   65 units: 16+1 x3, 0+14
  K=1040  split=8   65 units: 0+3 x21, 0+2, empty x10
  K=1536  split=1   96 units: 16+8 x4
  K=1536  split=3   96 units: 0+8 x12
  K=2032  split=1  127 units: 32+0 x3, 16+15
  K=2032  split=2  127 units: 16+0 x7, 0+15
  K=2048  split=1  128 units: 32+0 x4
  K=2048  split=4  128 units: 0+8 x16
  K=3056  split=1  191 units: 48+0 x3, 32+15
  K=3056  split=3  191 units: 16+0 x11, 0+15
  K=3072  split=1  192 units: 48+0 x4
  K=3072  split=8  192 units: 0+6 x32
  K=4096  split=1  256 units: 64+0 x4
  K=4096  split=2  256 units: 32+0 x8
  K=11008 split=1  688 units: 160+12 x4
  K=11008 split=4  688 units: 32+11 x16
decode_gemm U=12  (K = 1600 and 4608 are there for tail 1, the empty
                   waves and k-slice, and three pairs)
  K=1536  split=1   96 units: 24+0 x4
  K=1536  split=2   96 units: 0+12 x8
  K=1600  split=1  100 units: 24+1 x4
  K=1600  split=8  100 units: 0+4 x25, empty x7
  K=2048  split=1  128 units: 24+8 x4
  K=2048  split=3  128 units: 0+11 x11, 0+7
  K=3056  split=1  191 units: 48+0 x3, 24+23
  K=3056  split=2  191 units: 24+0 x7, 0+23
  K=3072  split=1  192 units: 48+0 x4
  K=3072  split=8  192 units: 0+6 x32
  K=4608  split=1  288 units: 72+0 x4
  K=4608  split=2  288 units: 24+12 x8
  K=11008 split=1  688 units: 168+4 x4
  K=11008 split=4  688 units: 24+19 x16
decode_gemm_w4 U=4  (K = 6144 is there for three pairs)
  K=64    split=1    1 units: 0+1, empty x3
  K=64    split=8    1 units: 0+1, empty x31
  K=832   split=1   13 units: 0+4 x3, 0+1
  K=832   split=2   13 units: 0+2 x6, 0+1, empty
  K=2048  split=1   32 units: 8+0 x4
  K=2048  split=3   32 units: 0+3 x10, 0+2, empty
  K=2112  split=1   33 units: 8+1 x3, 0+6
  K=2112  split=8   33 units: 0+2 x16, 0+1, empty x15
  K=4032  split=1   63 units: 16+0 x3, 8+7
  K=4032  split=2   63 units: 8+0 x7, 0+7
  K=4096  split=1   64 units: 16+0 x4
  K=4096  split=3   64 units: 0+6 x10, 0+4, empty
  K=6144  split=1   96 units: 24+0 x4
  K=6144  split=2   96 units: 8+4 x8
gemm_w4 has no ring over ranges: K = 64 .. 320 and 832 are 1 to 5 and 13
groups through its "W two groups ahead, x one ahead" pipeline.
"""
import functools

import pytest
import torch

from runbooks_amd import ops

from test_decode_gemm_exact_cpu import (
    BF16_U8_CASES, BF16_U12_CASES, GEMM_W4_CASES, GEMM_W4_NEEDLE,
    W4_DECODE_CASES, boundary_ks, exact_case_bf16_full, exact_case_w4,
    needle_batches, needle_case, needle_case_w4, swizzle_w_mirror,
    swizzle_x_mirror)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POISON = 1e3          # finite on purpose: a wrong kernel must give a wrong
#                       number, never a fault


def ext():
    assert ops.has_hip(), "gfx950 extension not loaded"
    return ops.ext()


bf16_case = functools.lru_cache(maxsize=None)(exact_case_bf16_full)
w4_case = functools.lru_cache(maxsize=None)(exact_case_w4)


def assert_bits(got, want, ks=None, what=""):
    """Bit equality; on failure the count of differing outputs and the
    first few (m, n, got, want), with the probed k for needle cases."""
    got = got.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, \
        (what, got.shape, got.dtype, want.shape, want.dtype)
    bits = torch.int16 if want.dtype == torch.bfloat16 else torch.int32
    bad = (got.contiguous().view(bits) !=
           want.contiguous().view(bits)).nonzero()
    if len(bad) == 0:
        return
    lines = [f"{what}: {len(bad)} of {want.numel()} outputs differ"]
    for idx in bad[:8].tolist():
        m, n = idx[-2], idx[-1]
        line = f"  (m={m}, n={n}) got {float(got[tuple(idx)])} " \
               f"want {float(want[tuple(idx)])}"
        if ks is not None:
            line += f"  k={ks[m]} (k-step {ks[m] // 16}, group {ks[m] // 64})"
        lines.append(line)
    pytest.fail("\n".join(lines))


def run_bf16(x, w, split=-1, u=0, layout=0, hq=0, hkv=0, dh=0, xs=None):
    e = ext()
    M, K = x.shape
    N = w.shape[0]
    ws = e.decode_swizzle_w_layout(w.to(DEV), layout, hq, hkv, dh)
    if xs is None:
        xs = e.decode_swizzle_x(x.to(DEV))
    return e.decode_gemm(xs, ws, M, N, K, split, layout, hq, hkv, dh, u)


def run_w4(x, q, s, split=-1, xs=None):
    e = ext()
    M, K = x.shape
    wq_swz, sc_swz = e.w4_swizzle(q.to(DEV), s.to(DEV))
    if xs is None:
        xs = e.decode_swizzle_x(x.to(DEV))
    return e.decode_gemm_w4(xs, wq_swz, sc_swz, M, q.shape[0], K, split)


def _partitions(cases):
    return sorted({(c.K, c.split) for c in cases})


# --------------------------------------------------------------------------
# decode_gemm (bf16), U = 8 and U = 12
# --------------------------------------------------------------------------
@pytest.mark.parametrize("c", BF16_U8_CASES, ids=lambda c: c.id)
def test_decode_gemm_exact(c):
    x, w, _, y_ref = bf16_case(c.M, c.N, c.K, c.seed)
    assert_bits(run_bf16(x, w, c.split), y_ref, what=c.id)


@pytest.mark.parametrize("c", BF16_U12_CASES, ids=lambda c: c.id)
def test_decode_gemm_u12_exact(c):
    x, w, _, y_ref = bf16_case(c.M, c.N, c.K, c.seed)
    assert_bits(run_bf16(x, w, c.split, u=12), y_ref, what=c.id + "-u12")


def _needles_bf16(K, split, U):
    e = ext()
    ws = None
    for ks in needle_batches(boundary_ks(K, split, U)):
        x, w, y = needle_case(32, 32, K, ks)
        if ws is None:                    # w depends on (N, K, seed) alone
            ws = e.decode_swizzle_w(w.to(DEV))
        got = e.decode_gemm(e.decode_swizzle_x(x.to(DEV)), ws, 32, 32, K,
                            split, u=0 if U == 8 else U)
        assert_bits(got, y, ks, f"needle K={K} split={split} U={U}")


@pytest.mark.parametrize("K,split", _partitions(BF16_U8_CASES))
def test_decode_gemm_needles(K, split):
    _needles_bf16(K, split, 8)


@pytest.mark.parametrize("K,split", _partitions(BF16_U12_CASES))
def test_decode_gemm_u12_needles(K, split):
    _needles_bf16(K, split, 12)


def test_decode_gemm_refuses_bad_split_and_u():
    x, w, _, _ = bf16_case(1, 32, 1024, 0)
    with pytest.raises(RuntimeError, match="force_split"):
        run_bf16(x, w, 9)
    with pytest.raises(RuntimeError, match="u must be"):
        run_bf16(x, w, 1, u=7)
    torch.cuda.synchronize()


# --------------------------------------------------------------------------
# swizzles against the mirror
# --------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 17, 32])
def test_decode_swizzle_x_matches_mirror(M):
    x, _, _, _ = bf16_case(M, 32, 1040, 0)
    got = ext().decode_swizzle_x(x.to(DEV))
    assert_bits(got.view(65, 64, 8), swizzle_x_mirror(x), what=f"xs M={M}")


def test_decode_swizzle_w_matches_mirror():
    _, w, _, _ = bf16_case(1, 96, 1040, 0)
    got = ext().decode_swizzle_w(w.to(DEV))
    assert_bits(got.reshape(3, 65, 64, 8), swizzle_w_mirror(w), what="ws")


# --------------------------------------------------------------------------
# padding lanes of the operand may hold anything finite
# --------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 17, 31])
def test_poisoned_operand_padding(M):
    """The fused GLU epilogue leaves the lanes m >= M of the operand it
    writes untouched. Finite poison there must not move a bit of
    decode_gemm (split 1, slabs, U = 12), decode_gemm_raw (bf16 and slab
    output) or decode_gemm_w4 (split 1 and slabs)."""
    e = ext()

    def poisoned(x):
        xs = swizzle_x_mirror(x, POISON)
        assert int((xs == POISON).sum()) == (32 - M) * x.shape[1]
        return xs.reshape(-1).to(DEV)

    x, w, _, y_ref = bf16_case(M, 96, 1040, 0)
    for split, u in ((1, 0), (3, 0), (1, 12), (8, 12)):
        clean = run_bf16(x, w, split, u)
        got = run_bf16(x, w, split, u, xs=poisoned(x))
        assert_bits(got, clean.cpu(), what=f"poison M={M} s={split} u={u}")
        assert_bits(got, y_ref, what=f"poison/ref M={M} s={split} u={u}")

    for N, K in ((96, 1536), (32, 4096)):          # raw: bf16, then slabs
        x, w, _, _ = bf16_case(M, N, K, 0)
        ws = e.decode_swizzle_w(w.to(DEV))
        clean = e.decode_gemm_raw(e.decode_swizzle_x(x.to(DEV)), ws, M, N, K)
        got = e.decode_gemm_raw(poisoned(x), ws, M, N, K)
        assert_bits(got, clean.cpu(), what=f"poison raw M={M} {N}x{K}")

    x, q, s, _, y_ref = w4_case(M, 96, 832, 0)
    for split in (1, 2):
        clean = run_w4(x, q, s, split)
        got = run_w4(x, q, s, split, xs=poisoned(x))
        assert_bits(got, clean.cpu(), what=f"poison w4 M={M} s={split}")
        assert_bits(got, y_ref, what=f"poison w4/ref M={M} s={split}")


# --------------------------------------------------------------------------
# decode_gemm_raw
# --------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 17, 32])
def test_decode_gemm_raw(M):
    """Split 1 returns y bf16; a split > 1 returns fp32 slabs whose sum is
    the exact product (which slice holds which k-range is not asserted:
    the consumer only sums them)."""
    e = ext()
    assert e.decode_gemm_split(96, 1536) == 1
    x, w, _, y_ref = bf16_case(M, 96, 1536, 0)
    y = e.decode_gemm_raw(e.decode_swizzle_x(x.to(DEV)),
                          e.decode_swizzle_w(w.to(DEV)), M, 96, 1536)
    assert_bits(y, y_ref, what=f"raw split 1 M={M}")

    split = e.decode_gemm_split(32, 4096)
    assert split > 1
    x, w, y32, _ = bf16_case(M, 32, 4096, 0)
    slabs = e.decode_gemm_raw(e.decode_swizzle_x(x.to(DEV)),
                              e.decode_swizzle_w(w.to(DEV)), M, 32, 4096)
    assert slabs.dtype == torch.float32 and slabs.shape == (split, M, 32)
    assert_bits(slabs.sum(0), y32, what=f"raw slabs M={M}")
    assert_bits(slabs.cpu().double().sum(0).float(), y32,
                what=f"raw slabs (f64 sum) M={M}")


# --------------------------------------------------------------------------
# layout tags: permuted weight rows, y in the original column order
# --------------------------------------------------------------------------
@pytest.mark.parametrize("layout,N,heads", [
    (1, 64, (0, 0, 0)),           # glu16, I = 32
    (2, 96, (1, 1, 32)),          # rope16, one block per head
    (2, 256, (2, 1, 64)),         # rope16, two blocks per head, GQA
])
@pytest.mark.parametrize("split", [1, 2])
def test_layout_tags_exact(layout, N, heads, split):
    x, w, _, y_ref = bf16_case(17, N, 1040, 0)
    got = run_bf16(x, w, split, 0, layout, *heads)
    assert_bits(got, y_ref, what=f"layout {layout} N={N} split={split}")


# --------------------------------------------------------------------------
# decode_gemm_w4
# --------------------------------------------------------------------------
@pytest.mark.parametrize("c", W4_DECODE_CASES, ids=lambda c: c.id)
def test_decode_gemm_w4_exact(c):
    x, q, s, _, y_ref = w4_case(c.M, c.N, c.K, c.seed)
    assert_bits(run_w4(x, q, s, c.split), y_ref, what=c.id)


@pytest.mark.parametrize("K,split", _partitions(W4_DECODE_CASES))
def test_decode_gemm_w4_needles(K, split):
    for ks in needle_batches(boundary_ks(K, split, 4, 64, clamp=True)):
        x, q, s, y = needle_case_w4(32, 32, K, ks)
        assert_bits(run_w4(x, q, s, split), y, ks,
                    f"w4 needle K={K} split={split}")


# --------------------------------------------------------------------------
# gemm_w4
# --------------------------------------------------------------------------
def run_gemm_w4(x, q, s):
    e = ext()
    wq_swz, sc_swz = e.w4_swizzle(q.to(DEV), s.to(DEV))
    return e.gemm_w4(x.to(DEV), wq_swz, sc_swz, q.shape[0], x.shape[1])


@pytest.mark.parametrize("M,N,K,seed", GEMM_W4_CASES)
def test_gemm_w4_exact(M, N, K, seed):
    x, q, s, _, y_ref = w4_case(M, N, K, seed)
    assert_bits(run_gemm_w4(x, q, s), y_ref, what=f"gemm_w4 {M}x{N}x{K}")


def test_gemm_w4_needle():
    """First and last k of each of the five groups, then a stride through
    the rest, over all three m-tiles of the MT = 4 kernel and its one
    ragged row."""
    M, N, K = GEMM_W4_NEEDLE
    ks = boundary_ks(K, 1, 1, 64, clamp=True)
    assert len(ks) == 2 * (K // 64)
    ks = ks + [(37 * m + 5) % K for m in range(M - len(ks))]
    x, q, s, y = needle_case_w4(M, N, K, ks)
    assert_bits(run_gemm_w4(x, q, s), y, ks, "gemm_w4 needle")
