"""The K tail of decode_gemm and decode_gemm_w4 through the ring, against
exact arithmetic and against the one-step tail loop, tolerance zero.

Cases and their reasons: test_decode_gemm_tail_cpu.py. Every case runs
with tail = 1 (the ring tail) and tail = 0 (the old loop); both must give
bf16_rne(exact sum) bit for bit, and so the same bits as each other.
Needles probe the first and last k of tail chunk 1 and of tail chunk 2 of
every wave. decode_gemm_raw and the fused glu / rope entry points take
their tail from RB_DG_TAIL, read once per process: one fresh child process
runs them with the other setting and every output tensor is compared with
torch.equal. The poison cases put finite garbage where a clamp that runs
one unit past a wave's end would read it: in W behind a wave's last step
(x zero there, so the true product ignores it), in x likewise, and in the
memory behind the last step of either operand.
"""
import functools
import os
import subprocess
import sys

import pytest
import torch

from runbooks_amd import ops

from test_decode_gemm_exact_cpu import (
    exact_case_bf16_full, exact_case_w4, needle_case, needle_case_w4,
    wave_range)
from test_decode_gemm_exact_gpu import assert_bits
from test_decode_gemm_tail_cpu import (
    NEEDLE_U8, NEEDLE_U12, NEEDLE_W4, TAIL_EDGES, TAIL_U8, TAIL_U12,
    TAIL_W4, tail_chunk_ks)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POISON = 1e3          # finite: a wrong kernel gives a wrong number, no fault
TAILS = (1, 0)


def ext():
    assert ops.has_hip(), "gfx950 extension not loaded"
    return ops.ext()


bf16_case = functools.lru_cache(maxsize=None)(exact_case_bf16_full)
w4_case = functools.lru_cache(maxsize=None)(exact_case_w4)


def run_bf16(x, w, split, U, tail, layout=0, heads=(0, 0, 0)):
    e = ext()
    M, K = x.shape
    N = w.shape[0]
    ws = e.decode_swizzle_w_layout(w.to(DEV), layout, *heads)
    xs = e.decode_swizzle_x(x.to(DEV))
    return e.decode_gemm(xs, ws, M, N, K, split, layout, *heads,
                         0 if U == 8 else U, tail)


def run_w4(x, q, s, split, tail):
    e = ext()
    M, K = x.shape
    wq_swz, sc_swz = e.w4_swizzle(q.to(DEV), s.to(DEV))
    xs = e.decode_swizzle_x(x.to(DEV))
    return e.decode_gemm_w4(xs, wq_swz, sc_swz, M, q.shape[0], K, split, tail)


def _both_tails_exact(c, U):
    x, w, _, y_ref = bf16_case(c.M, c.N, c.K, c.seed)
    got = {t: run_bf16(x, w, c.split, U, t) for t in TAILS}
    for t in TAILS:
        assert_bits(got[t], y_ref, what=f"{c.id} U={U} tail={t}")
    assert torch.equal(got[1], got[0])


@pytest.mark.parametrize("c", TAIL_U8, ids=lambda c: c.id)
def test_tail_sweep_u8(c):
    _both_tails_exact(c, 8)


@pytest.mark.parametrize("c", TAIL_U12, ids=lambda c: c.id)
def test_tail_sweep_u12(c):
    _both_tails_exact(c, 12)


@pytest.mark.parametrize("c,U", TAIL_EDGES,
                         ids=lambda v: v.id if hasattr(v, "id") else f"U{v}")
def test_tail_edges(c, U):
    _both_tails_exact(c, U)


@pytest.mark.parametrize("shape", [NEEDLE_U8, NEEDLE_U12],
                         ids=["U8", "U12"])
def test_tail_chunk_needles(shape):
    K, split, U, unit_k, clamp = shape
    ks = tail_chunk_ks(K, split, U, unit_k, clamp)
    ks = ks + [ks[-1]] * (32 - len(ks))
    x, w, y = needle_case(32, 32, K, ks)
    for t in TAILS:
        assert_bits(run_bf16(x, w, split, U, t), y, ks,
                    f"needle K={K} U={U} tail={t}")


# --------------------------------------------------------------------------
# the entry points that take their tail from RB_DG_TAIL alone
# --------------------------------------------------------------------------
ENV_K = 1024 + 64 * 13       # 16 + 13 steps per wave: both tail chunks
ENV_M = 17


def _rope_inputs(hq, hkv, dh, vt):
    n = (hq + 2 * hkv) * dh
    x, w, _, _ = bf16_case(ENV_M, n, ENV_K, 0)
    w = (w.float() / 64).to(torch.bfloat16)      # exact: keeps RoPE finite
    cos, sin = (t.to(DEV) for t in ops.rope_tables(dh, 64, 10000.0))
    pos = torch.tensor([(37 * i + 5) % 61 for i in range(ENV_M)],
                       dtype=torch.int32, device=DEV)
    slots = torch.tensor([ops.BLOCK_SIZE + i for i in range(ENV_M)],
                         dtype=torch.int32, device=DEV)
    kc, vc = ops.alloc_kv_cache(4, hkv, dh, DEV, v_transposed=vt)
    kc.zero_()
    vc.zero_()
    return n, x, w, cos, sin, pos, slots, kc, vc


def env_entry_points():
    """Every output of decode_gemm_raw (slabs at K = 11008, N = 32, and a
    bf16 y), decode_gemm_glu (swiglu, geglu at the smallest N, I = 16) and
    decode_gemm_rope_append (plain and transposed-V cache at the smallest
    heads, N = 192) on fixed inputs, on the CPU. Their tail is whatever
    RB_DG_TAIL says in this process."""
    e = ext()
    out = {}
    for M in (1, 17, 32):
        x, w, _, _ = bf16_case(M, 32, 11008, 0)
        out[f"raw_slabs_M{M}"] = e.decode_gemm_raw(
            e.decode_swizzle_x(x.to(DEV)), e.decode_swizzle_w(w.to(DEV)),
            M, 32, 11008)
    x, w, _, _ = bf16_case(ENV_M, 96, ENV_K, 0)       # split 1: bf16 y
    out["raw_y"] = e.decode_gemm_raw(
        e.decode_swizzle_x(x.to(DEV)), e.decode_swizzle_w(w.to(DEV)),
        ENV_M, 96, ENV_K)
    x, w, _, _ = bf16_case(ENV_M, 32, ENV_K, 0)
    xs = e.decode_swizzle_x(x.to(DEV))
    ws = e.decode_swizzle_w_layout(w.to(DEV), 1)
    for gelu in (False, True):
        swz = e.decode_gemm_glu(xs, ws, ENV_M, 32, ENV_K, gelu)
        out[f"glu_gelu{int(gelu)}"] = \
            swz.view(-1, 2, 32, 8)[:, :, :ENV_M].contiguous()
    for vt in (False, True):
        hq, hkv, dh = (4, 1, 64) if vt else (1, 1, 64)
        n, x, w, cos, sin, pos, slots, kc, vc = _rope_inputs(hq, hkv, dh, vt)
        q = e.decode_gemm_rope_append(
            e.decode_swizzle_x(x.to(DEV)),
            e.decode_swizzle_w_layout(w.to(DEV), 2, hq, hkv, dh), ENV_M, n,
            ENV_K, cos, sin, pos, kc, vc, slots, hq)
        out.update({f"rope_q_vt{int(vt)}": q, f"rope_k_vt{int(vt)}": kc,
                    f"rope_v_vt{int(vt)}": vc})
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


@pytest.fixture(scope="module")
def other_tail(tmp_path_factory):
    """env_entry_points() of a fresh child process whose RB_DG_TAIL picks
    the tail this process does not use (the variable is read once)."""
    here = os.path.dirname(os.path.abspath(__file__))
    path = str(tmp_path_factory.mktemp("tail") / "child.pt")
    mine = "0" if os.environ.get("RB_DG_TAIL") == "0" else "1"
    env = dict(os.environ, RB_DG_TAIL="1" if mine == "0" else "0")
    code = ("import sys, torch; sys.path[:0] = [%r, %r]; "
            "import test_decode_gemm_tail_gpu as t; "
            "torch.save(t.env_entry_points(), %r)"
            % (here, os.path.dirname(here), path))
    subprocess.run([sys.executable, "-c", code], env=env, check=True,
                   timeout=120)
    return torch.load(path)


def test_env_entry_points_equal_between_tails(other_tail):
    """The raw slabs themselves (not their sum), the bf16 y, the fused glu
    operand and the fused rope q / k cache / v cache are the same tensors
    with RB_DG_TAIL=0 and without."""
    mine = env_entry_points()
    assert set(mine) == set(other_tail) and len(mine) == 12
    assert mine["raw_slabs_M17"].shape == (8, 17, 32)
    assert mine["raw_slabs_M17"].dtype == torch.float32
    assert mine["raw_y"].shape == (17, 96)
    for name, t in mine.items():
        assert float(t.float().abs().max()) > 0, name
        assert t.dtype == other_tail[name].dtype and \
            torch.equal(t, other_tail[name]), name


def test_raw_slabs_sum_to_the_exact_product():
    """K = 11008 at N = 32 makes the split 8: 22 steps per wave = 16 + 6,
    the last wave 6."""
    e = ext()
    split = e.decode_gemm_split(32, 11008)
    assert split == 8
    for M in (1, 17, 32):
        x, w, y32, y_ref = bf16_case(M, 32, 11008, 0)
        xs = e.decode_swizzle_x(x.to(DEV))
        ws = e.decode_swizzle_w(w.to(DEV))
        slabs = e.decode_gemm_raw(xs, ws, M, 32, 11008)
        assert slabs.dtype == torch.float32 and slabs.shape == (split, M, 32)
        assert_bits(slabs.sum(0), y32, what=f"raw slabs M={M}")
        for t in TAILS:
            assert_bits(e.decode_gemm(xs, ws, M, 32, 11008, tail=t), y_ref,
                        what=f"combined M={M} tail={t}")


@pytest.mark.parametrize("layout,N,heads", [
    (1, 64, (0, 0, 0)),           # glu16, I = 32
    (2, 96, (1, 1, 32)),          # rope16, one block per head
])
@pytest.mark.parametrize("split", [1, 2])
def test_unpermuting_stores_equal_between_tails(layout, N, heads, split):
    K = 1856 * split              # 16 + 13 steps per wave at either split
    x, w, _, y_ref = bf16_case(17, N, K, 0)
    got = {t: run_bf16(x, w, split, 8, t, layout, heads) for t in TAILS}
    for t in TAILS:
        assert_bits(got[t], y_ref, what=f"layout {layout} s={split} tail={t}")
    assert torch.equal(got[1], got[0])


@pytest.mark.parametrize("gelu", [False, True], ids=["swiglu", "geglu"])
def test_fused_glu_epilogue_over_a_tail(gelu):
    """Smallest glu16 N (I = 16), K with both tail chunks: the fused
    epilogue equals the packed kernel over decode_gemm with either tail."""
    e = ext()
    x, w, _, _ = bf16_case(ENV_M, 32, ENV_K, 0)
    xs = e.decode_swizzle_x(x.to(DEV))
    swz = e.decode_gemm_glu(xs, e.decode_swizzle_w_layout(w.to(DEV), 1),
                            ENV_M, 32, ENV_K, gelu)
    for t in TAILS:
        y = e.decode_gemm(xs, e.decode_swizzle_w(w.to(DEV)), ENV_M, 32, ENV_K,
                          tail=t)
        _, ref = (e.geglu_packed_dec if gelu else e.swiglu_packed_dec)(y)
        assert torch.equal(swz.view(-1, 2, 32, 8)[:, :, :ENV_M],
                           ref.view(-1, 2, 32, 8)[:, :, :ENV_M]), t


@pytest.mark.parametrize("vt", [False, True], ids=["plain", "vt"])
def test_fused_rope_epilogue_over_a_tail(vt):
    e = ext()
    hq, hkv, dh = (4, 1, 64) if vt else (1, 1, 64)
    n, x, w, cos, sin, pos, slots, kc, vc = _rope_inputs(hq, hkv, dh, vt)
    assert (vc.shape[2] == dh and vc.shape[3] != dh) == vt
    xs = e.decode_swizzle_x(x.to(DEV))
    q = e.decode_gemm_rope_append(
        xs, e.decode_swizzle_w_layout(w.to(DEV), 2, hq, hkv, dh), ENV_M, n,
        ENV_K, cos, sin, pos, kc, vc, slots, hq)
    for t in TAILS:
        y = e.decode_gemm(xs, e.decode_swizzle_w(w.to(DEV)), ENV_M, n, ENV_K,
                          tail=t)
        kr, vr = torch.zeros_like(kc), torch.zeros_like(vc)
        qr = e.qkv_rope_append(y, cos, sin, pos, kr, vr, slots, hq)
        assert torch.equal(q, qr) and torch.equal(kc, kr) and \
            torch.equal(vc, vr), t


# --------------------------------------------------------------------------
# poison where an overrunning clamp would read
# --------------------------------------------------------------------------
def _wave_ends(K, split, unit_k=16, clamp=False):
    """First unit after each non-empty wave's range, where one exists."""
    units = K // unit_k
    ends = set()
    for g in range(4 * split):
        u0, u1 = wave_range(units, split, g, clamp)
        if u1 > u0 and u1 < units:
            ends.add(u1)
    return sorted(ends)


@pytest.mark.parametrize("K,split,U", [(1024 + 64 * 6, 1, 8),
                                       (1024 + 64 * 13, 1, 8),
                                       (1600, 4, 8), (11008, 2, 8),
                                       (1536 + 64 * 17, 1, 12)])
def test_poison_catches_a_one_sided_overrun(K, split, U):
    """Step u1 of a wave is step u0 of the next. With x zero over that
    step and W poisoned there (then the other way round), the true product
    does not see the poison; a load that runs one step past u1 while its
    partner is clamped does. An overrun of both operands multiplies the
    poison by the zero and is not seen here: it counts a real step twice,
    which the exact sums of the sweeps catch."""
    M, N = 17, 32
    x, w, _, _ = bf16_case(M, N, K, 0)
    cols = torch.tensor([s * 16 + i for s in _wave_ends(K, split)
                         for i in range(16)])
    assert len(cols)
    for poison_w in (True, False):
        xp, wp = x.clone(), w.clone()
        (wp if poison_w else xp)[:, cols] = POISON
        (xp if poison_w else wp)[:, cols] = 0.0
        y = (xp.double() @ wp.double().t()).float()
        assert torch.equal(y.double(), xp.double() @ wp.double().t())
        for t in TAILS:
            assert_bits(run_bf16(xp, wp, split, U, t), y.to(torch.bfloat16),
                        what=f"poison {'w' if poison_w else 'x'} K={K} "
                             f"s={split} U={U} tail={t}")


@pytest.mark.parametrize("K,split,U", [(1024 + 64 * 6, 1, 8),
                                       (1600, 4, 8), (1536 + 64 * 17, 1, 12)])
def test_poison_behind_the_operands(K, split, U):
    """Both operands are views of larger buffers whose remainder is
    poison: the last wave's clamp must stop at the last real step."""
    e = ext()
    M, N = 17, 32
    x, w, _, y_ref = bf16_case(M, N, K, 0)
    pad = 4 * 512
    xs_big = torch.full(((K // 16) * 512 + pad,), POISON,
                        dtype=torch.bfloat16, device=DEV)
    ws_big = torch.full((N * K + pad,), POISON, dtype=torch.bfloat16,
                        device=DEV)
    xs, ws = xs_big[:(K // 16) * 512], ws_big[:N * K]
    xs.copy_(e.decode_swizzle_x(x.to(DEV)).reshape(-1))
    ws.copy_(e.decode_swizzle_w(w.to(DEV)).reshape(-1))
    for t in TAILS:
        got = e.decode_gemm(xs, ws, M, N, K, split, 0, 0, 0, 0,
                            0 if U == 8 else U, t)
        assert_bits(got, y_ref, what=f"pad poison K={K} s={split} tail={t}")
    assert bool((xs_big[-pad:] == POISON).all())


# --------------------------------------------------------------------------
# decode_gemm_w4: the same sweep over groups
# --------------------------------------------------------------------------
@pytest.mark.parametrize("c", TAIL_W4, ids=lambda c: c.id)
def test_w4_tail_sweep(c):
    x, q, s, _, y_ref = w4_case(c.M, c.N, c.K, c.seed)
    got = {t: run_w4(x, q, s, c.split, t) for t in TAILS}
    for t in TAILS:
        assert_bits(got[t], y_ref, what=f"w4 {c.id} tail={t}")
    assert torch.equal(got[1], got[0])


def test_w4_tail_chunk_needles():
    K, split, U, unit_k, clamp = NEEDLE_W4
    ks = tail_chunk_ks(K, split, U, unit_k, clamp)
    ks = ks + [ks[-1]] * (32 - len(ks))
    x, q, s, y = needle_case_w4(32, 32, K, ks)
    for t in TAILS:
        assert_bits(run_w4(x, q, s, split, t), y, ks,
                    f"w4 needle K={K} tail={t}")


def test_w4_poison_behind_the_operands():
    e = ext()
    M, N, K = 17, 32, 2048 + 256 * 6
    x, q, s, _, y_ref = w4_case(M, N, K, 0)
    wq, sc = e.w4_swizzle(q.to(DEV), s.to(DEV))
    pad = 4096
    xs_big = torch.full(((K // 16) * 512 + pad,), POISON,
                        dtype=torch.bfloat16, device=DEV)
    wq_big = torch.full((wq.numel() + pad,), 0x7F, dtype=torch.uint8,
                        device=DEV)
    sc_big = torch.full((sc.numel() + pad,), POISON, dtype=torch.bfloat16,
                        device=DEV)
    xs = xs_big[:(K // 16) * 512]
    xs.copy_(e.decode_swizzle_x(x.to(DEV)).reshape(-1))
    wq_v = wq_big[:wq.numel()].view(wq.shape)
    wq_v.copy_(wq)
    sc_v = sc_big[:sc.numel()].view(sc.shape)
    sc_v.copy_(sc)
    for t in TAILS:
        got = e.decode_gemm_w4(xs, wq_v, sc_v, M, N, K, 1, t)
        assert_bits(got, y_ref, what=f"w4 pad poison tail={t}")
