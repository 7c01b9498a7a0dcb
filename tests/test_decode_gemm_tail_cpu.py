"""The K tail of the decode GEMMs: case tables for the GPU module and a
mirror of the ring tail's walk.

decode_gemm.hip and decode_gemm_w4.hip run the t = n % 2U units that the
ring pairs leave over (n = units of one wave) either one at a time (the
old loop, tail = 0) or through the ring: tail chunk 1 (t1 = min(t, U)
units) is loaded into the A half under the last B chunk's MFMAs, chunk 2
(t2 = t - t1) into the B half, each as U loads whose unit index is clamped
to the wave's last real unit. The partition into waves is the same either
way, and so is the order in which units are consumed.

Checked here without a GPU:
  * waves(K, split, U) of the existing mirror is what it was;
  * the tables used by test_decode_gemm_tail_gpu.py reach t = 0..15 at
    U = 8, t = 0..23 at U = 12 and t = 0..7 at U = 4 (w4, in groups), a
    short last wave, an empty wave, a tail-only wave and the production
    shape (K = 11008 at split 2: 86 steps per wave, tail 6);
  * ring_tail_walk (the new kernel branch by branch) consumes each wave's
    units once, in ascending order, and no load leaves the wave's range.
"""
import pytest

from test_decode_gemm_exact_cpu import (
    Case, exact_case_bf16_full, exact_case_w4, partition, ring_visit,
    wave_range)


def waves(K, split, U, unit_k=16, clamp=False):
    return [(m, t) for _, _, m, t, _ in
            partition(K // unit_k, split, U, clamp)]


# --------------------------------------------------------------------------
# tables (the GPU module runs exactly these)
# --------------------------------------------------------------------------
_MS = (1, 17, 32)
_NS = (32, 96)

# K = 1024 + 64 t at split 1: 16 + t steps per wave, tail t = 0..15
TAIL_U8 = [Case(_MS[t % 3], _NS[t % 2], 1024 + 64 * t, 1)
           for t in range(16)]
# K = 1536 + 64 t at split 1: 24 + t steps per wave, tail t = 0..23
TAIL_U12 = [Case(_MS[t % 3], _NS[t % 2], 1536 + 64 * t, 1)
            for t in range(24)]
# (case, U): the production down-proj shape at its own split and at 1,
# short and empty waves (K = 1600: 100 steps; split 4 gives 7 per wave,
# the last two waves 2 and none; split 8 gives 4 per wave and 7 empty
# waves), and 2 steps per wave (all tail)
TAIL_EDGES = [(Case(32, 32, 11008, 2), 8), (Case(17, 32, 11008, 1), 8),
              (Case(1, 32, 11008, 2), 12),
              (Case(17, 96, 1600, 4), 8), (Case(32, 32, 1600, 8), 8),
              (Case(1, 96, 1600, 4), 12), (Case(32, 96, 1024, 8), 8)]
# w4, units are groups of 64 k, U = 4: K = 2048 + 256 t at split 1 gives
# 8 + t groups per wave, t = 0..7; then uneven and empty ranges and the
# down-proj shape at its own split (172 groups over 16 waves: 8 + 3)
TAIL_W4 = [Case(_MS[t % 3], _NS[t % 2], 2048 + 256 * t, 1)
           for t in range(8)] + \
    [Case(32, 32, 11008, 4), Case(17, 96, 2112, 1), Case(1, 32, 2112, 8),
     Case(32, 96, 832, 2), Case(17, 32, 64, 1)]

# needle shapes: (K, split, U, unit_k, clamp) with both tail chunks present
NEEDLE_U8 = (1024 + 64 * 12, 1, 8, 16, False)      # 16 + 8 + 4 per wave
NEEDLE_U12 = (1536 + 64 * 20, 1, 12, 16, False)    # 24 + 12 + 8
NEEDLE_W4 = (2048 + 256 * 6, 1, 4, 64, True)       # 8 + 4 + 2 groups


def tail_chunk_ks(K, split, U, unit_k=16, clamp=False):
    """First k of the first unit and last k of the last unit of tail chunk
    1 and of tail chunk 2, for every wave that has them."""
    ks = []
    for g in range(4 * split):
        u0, u1 = wave_range(K // unit_k, split, g, clamp)
        n = max(u1 - u0, 0)
        t = n % (2 * U)
        base = u0 + n - t
        for lo, hi in ((base, base + min(t, U)), (base + U, u1)):
            if hi > lo:
                ks += [lo * unit_k, hi * unit_k - 1]
    return ks


# --------------------------------------------------------------------------
# the ring tail, branch by branch
# --------------------------------------------------------------------------
def ring_tail_walk(u0, u1, U):
    """-> (units in MFMA order, every unit index a load touches)."""
    out, loads = [], []
    n = u1 - u0
    nmain = (abs(n) // (2 * U)) * (2 * U) * (1 if n >= 0 else -1)
    smain = u0 + max(nmain, 0)
    t1, t2, last = min(u1 - smain, U), u1 - smain - U, u1 - 1
    ring = {}

    def load(half, base, clamp=False):
        ring[half] = [min(base + u, last) if clamp else base + u
                      for u in range(U)]
        loads.extend(ring[half])

    def mfma(half, cnt=U):
        out.extend(ring[half][:max(cnt, 0)])

    def tail():
        if t2 > 0:
            load("B", smain + U, True)
            mfma("A", t1)
            mfma("B", t2)
        else:
            mfma("A", t1)

    if nmain > 0:
        s = u0
        load("A", s)
        while s + 2 * U < smain:
            load("B", s + U)
            mfma("A")
            load("A", s + 2 * U)
            mfma("B")
            s += 2 * U
        load("B", s + U)
        mfma("A")
        if t1 > 0:
            load("A", smain, True)
            mfma("B")
            tail()
        else:
            mfma("B")
    elif t1 > 0:
        load("A", u0, True)
        tail()
    return out, loads


# --------------------------------------------------------------------------
# tests
# --------------------------------------------------------------------------
def test_partition_is_what_it_was():
    assert waves(11008, 2, 8) == [(80, 6)] * 8
    assert waves(11008, 2, 12) == [(72, 14)] * 8
    assert waves(11008, 1, 8) == [(160, 12)] * 4
    assert waves(4096, 2, 8) == [(32, 0)] * 8                   # o_proj
    assert waves(1600, 4, 8) == [(0, 7)] * 14 + [(0, 2), (0, 0)]
    assert waves(1600, 8, 8) == [(0, 4)] * 25 + [(0, 0)] * 7
    assert waves(1024, 8, 8) == [(0, 2)] * 32
    assert waves(11008, 4, 4, 64, True) == [(8, 3)] * 15 + [(0, 7)]
    # the last wave of K = 1600 at split 4 starts past the end
    u0, u1 = wave_range(100, 4, 15)
    assert (u0, u1) == (105, 100)


def test_tables_cover_every_tail_length():
    for t, c in enumerate(TAIL_U8):
        assert waves(c.K, c.split, 8) == [(16, t)] * 4
    for t, c in enumerate(TAIL_U12):
        assert waves(c.K, c.split, 12) == [(24, t)] * 4
    for t, c in enumerate(TAIL_W4[:8]):
        assert waves(c.K, c.split, 4, 64, True) == [(8, t)] * 4
    for cases in (TAIL_U8, TAIL_U12, TAIL_W4[:8]):
        assert {c.M for c in cases} == {1, 17, 32}
        assert {c.N for c in cases} == {32, 96}
    edges = {(c.K, c.split, U) for c, U in TAIL_EDGES}
    assert {(11008, 2, 8), (11008, 1, 8), (1600, 4, 8), (1600, 8, 8),
            (1024, 8, 8)} <= edges
    flags = set()
    for c, U in TAIL_EDGES:
        for main, tail in waves(c.K, c.split, U):
            flags.add("empty" if main + tail == 0 else
                      "tail-only" if main == 0 else "ring+tail")
        short = waves(c.K, c.split, U)
        if len({m + t for m, t in short if m + t}) > 1:
            flags.add("short last wave")
    assert flags == {"empty", "tail-only", "ring+tail", "short last wave"}
    w4 = [w for c in TAIL_W4 for w in waves(c.K, c.split, 4, 64, True)]
    assert (0, 0) in w4 and (0, 7) in w4 and (8, 3) in w4 and (0, 1) in w4


def test_every_case_is_exact():
    """The builders assert the 2^24 condition."""
    for c in [c for c, _ in TAIL_EDGES] + TAIL_U8[-1:] + TAIL_U12[-1:]:
        exact_case_bf16_full(c.M, c.N, c.K, c.seed)
    for c in TAIL_W4[7:]:
        exact_case_w4(c.M, c.N, c.K, c.seed)


@pytest.mark.parametrize("U", [4, 8, 12])
def test_ring_tail_walk_matches_the_old_order_and_stays_in_range(U):
    for n in range(-40, 100):
        u0, u1 = 5, 5 + n
        got, loads = ring_tail_walk(u0, u1, U)
        assert got == [u for _, u in ring_visit(u0, u1, U)] == \
            list(range(u0, max(u0, u1))), (U, n)
        assert all(u0 <= u < u1 for u in loads), (U, n)
        if n <= 0:
            assert not loads


def test_needle_positions():
    for K, split, U, unit_k, clamp in (NEEDLE_U8, NEEDLE_U12, NEEDLE_W4):
        ks = tail_chunk_ks(K, split, U, unit_k, clamp)
        assert len(ks) == 16 and len(set(ks)) == 16 and max(ks) == K - 1
    # wave 0 of the U = 8 shape: steps 16..23 and 24..27
    assert tail_chunk_ks(*NEEDLE_U8)[:4] == [256, 383, 384, 447]
