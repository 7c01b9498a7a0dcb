"""Exact-arithmetic cases for the weight-stream GEMMs, a CPU mirror of
ops/csrc/decode_gemm.hip's dataflow, and proof that the checks bite.

decode_gemm.hip, decode_gemm_w4.hip and gemm_w4.hip accumulate bf16 x bf16
products in fp32. The builders below choose inputs for which every product
and every partial sum of an output is an integer multiple of one power of
two (that output's quantum) below 2^24 quanta, so an fp32 sum of them is
exact in ANY order: ring depth, k-split, wave count and reduce tree cannot
move a bit, and the right answer is bf16_rne(exact sum). The GPU module
(test_decode_gemm_exact_gpu.py) imports the builders and the case lists
from here and compares with tolerance zero.

What this module checks without a GPU:
  * the 2^24 condition of every case (asserted inside the builders);
  * a mirror of the bf16 kernel (swizzles, per-(kslice, wave) step ranges,
    the main/tail ring partition for U = 8 / 12 including negative ranges,
    the MFMA A/B/C lane maps, the four-wave reduce, the slab combine)
    reproduces y_ref bit for bit; the same engine over groups of four
    k-steps with U = 4 mirrors decode_gemm_w4.hip from its stored bytes;
  * the ring partition visits each range once, and the case lists reach
    tail 0, 1 and 2U-1, a tail-only wave, an empty wave, an empty k-slice
    and 1, 2 and 3 ring pairs (the GPU module's docstring table is
    print_partition_table()'s output);
  * one lost, doubled or misplaced k-step, lane fragment, nibble or scale
    changes at least one output bit of every case, at the first, a middle
    and the last position: a kernel with such a fault fails the GPU checks.

Keep in sync with the three .hip files when editing any of them.
"""
import dataclasses

import numpy as np
import pytest
import torch

from runbooks_amd.ops import linear as L

from test_w4_cpu import w4_swizzle_mirror

F24 = 1 << 24


# --------------------------------------------------------------------------
# exact cases
# --------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randint(lo, hi, shape, g):
    return torch.randint(lo, hi + 1, shape, generator=g, dtype=torch.int64)


def _to_bf16_exact(v):
    """float64 -> bf16, asserting nothing is rounded away."""
    b = v.to(torch.float32).to(torch.bfloat16)
    assert torch.equal(b.to(torch.float64), v), "not representable in bf16"
    return b


def x_amplitude(K, wmax):
    """Largest |b| for which sum_k |b||a| < 2^24 whatever the draw."""
    return int(max(1, min(127, (F24 - 1) // (wmax * K))))


def _exact_x(M, K, A, g):
    b = _randint(-A, A, (M, K), g)
    xe = torch.arange(M) % 4 - 1
    x = _to_bf16_exact(b.double() * torch.exp2(xe.double())[:, None])
    return b, xe, x


def _exact_product(b, xe, a, we):
    """y = (b 2^xe) (a 2^we)^T for integer b [M,K], a [N,K] and per-row
    exponents. Asserts the exactness condition: for every output, sum_k
    |x||w| over that output's quantum 2^(xe[m] + we[n]) (every product, so
    every partial sum in any order, is a multiple of it; no smaller
    quantum is in play for that output) is below 2^24. Returns
    (y fp32 exact, y bf16 = the single RNE rounding of it)."""
    quanta = (b.abs() @ a.abs().t())                 # int64, exact
    assert int(quanta.max()) < F24, int(quanta.max())
    q = torch.exp2((xe[:, None] + we[None, :]).double())
    y = (b @ a.t()).double() * q
    y32 = y.to(torch.float32)
    assert torch.equal(y32.double(), y)
    return y32, y32.to(torch.bfloat16)


def exact_case_bf16(M, N, K, seed):
    """x [M,K], w [N,K] bf16 and y_ref [M,N] bf16 = bf16_rne(x w^T)."""
    x, w, _, y_ref = exact_case_bf16_full(M, N, K, seed)
    return x, w, y_ref


def exact_case_bf16_full(M, N, K, seed):
    """As exact_case_bf16, plus the exact fp32 product (for the slabs)."""
    g = _gen(seed)
    a = _randint(-127, 127, (N, K), g)
    we = torch.arange(N) % 5 - 2
    w = _to_bf16_exact(a.double() * torch.exp2(we.double())[:, None])
    b, xe, x = _exact_x(M, K, x_amplitude(K, 127), g)
    y32, y_ref = _exact_product(b, xe, a, we)
    return x, w, y32, y_ref


def w4_scale_exponents(N, G):
    """Exponent of the scale of (row n, group g): (3n + 2g) % 5 - 2.

    Not the (3n + 5g) % 5 first proposed for these cases: 5g vanishes mod
    5, so that scale would not depend on the group and a scale taken from
    group g+1 would be the same number. With 2g a neighbouring row (+3)
    and a neighbouring group (+2) are both a different power of two,
    which is what the scale mutation below needs."""
    n = torch.arange(N)[:, None]
    g = torch.arange(G)[None, :]
    return (3 * n + 2 * g) % 5 - 2


def exact_case_w4(M, N, K, seed):
    """x bf16 [M,K], canonical q uint8 [N,K/2], scales bf16 [N,K/64], the
    dequantized weight float64 [N,K] and y_ref bf16 [M,N]. q and the
    scales are built directly, never through quantize_int4."""
    g = _gen(seed)
    codes = _randint(-8, 7, (N, K), g)
    nib = (codes + 8).to(torch.uint8)
    q = (nib[:, 0::2] | (nib[:, 1::2] << 4)).contiguous()
    se = w4_scale_exponents(N, K // 64)
    scales = _to_bf16_exact(torch.exp2(se.double())).contiguous()
    wdq = (codes.reshape(N, K // 64, 64).double()
           * torch.exp2(se.double())[:, :, None]).reshape(N, K)
    assert torch.equal(
        L.dequantize_int4(q, scales, dtype=torch.bfloat16).double(), wdq)
    # per-output quantum: the smallest weight quantum of row n, 2^-2,
    # times the x quantum of row m
    a = (wdq * 4.0).to(torch.int64)
    b, xe, x = _exact_x(M, K, x_amplitude(K, 8 * 16), g)
    we = torch.full((N,), -2, dtype=torch.int64)
    _, y_ref = _exact_product(b, xe, a, we)
    return x, q, scales, wdq, y_ref


# --------------------------------------------------------------------------
# needle cases
# --------------------------------------------------------------------------
def needle_x(M, K, ks):
    assert len(ks) == M and all(0 <= k < K for k in ks)
    x = torch.zeros(M, K, dtype=torch.bfloat16)
    x[torch.arange(M), torch.tensor(list(ks))] = 1.0
    return x


def needle_case(M, N, K, ks, seed=0):
    """Row m of x is 1.0 at column ks[m]: y[m, n] == w[n, ks[m]]."""
    w = _randint(-127, 127, (N, K), _gen(seed)).to(torch.bfloat16)
    return needle_x(M, K, ks), w, w[:, list(ks)].t().contiguous()


def needle_case_w4(M, N, K, ks, seed=0):
    """The w4 exact case's weights under a needle x: y[m, n] is the
    dequantized weight [n, ks[m]] = code * scale, a bf16 number."""
    _, q, scales, wdq, _ = exact_case_w4(1, N, K, seed)
    y = _to_bf16_exact(wdq[:, list(ks)].t().contiguous())
    return needle_x(M, K, ks), q, scales, y


# --------------------------------------------------------------------------
# partition: wave ranges and the ring, as the kernels compute them
# --------------------------------------------------------------------------
def wave_range(units, split, g, clamp=False):
    """Unit range [u0, u1) of group g = kslice * 4 + wave. decode_gemm.hip
    (units = k-steps) leaves u0 unclamped, so u1 - u0 may be negative;
    decode_gemm_w4.hip (units = groups of 64 k) clamps u0."""
    per = (units + 4 * split - 1) // (4 * split)
    u0 = g * per
    if clamp:
        u0 = min(units, u0)
    return u0, min(units, u0 + per)


def _cdiv_trunc(a, b):
    return a // b if a >= 0 else -((-a) // b)


def ring_visit(u0, u1, U):
    """Units in the order the kernel's MFMAs consume them, with the part
    that feeds each: ('A' | 'B' | 'tail', unit). Follows the loop of
    decode_gemm_kernel branch by branch; each MFMA chunk consumes what its
    ring half LAST LOADED, so a stale or skipped reload shows."""
    out = []
    s = u0
    nmain = _cdiv_trunc(u1 - u0, 2 * U) * (2 * U)    # C division truncates
    if nmain > 0:
        ring = {"A": s, "B": None}
        smain = u0 + nmain
        while s + 2 * U <= smain:
            if s + U < smain:
                ring["B"] = s + U
            out += [("A", ring["A"] + u) for u in range(U)]
            if s + 2 * U < smain:
                ring["A"] = s + 2 * U
            if s + U < smain:
                out += [("B", ring["B"] + u) for u in range(U)]
            s += 2 * U
    while s < u1:
        out.append(("tail", s))
        s += 1
    return out


def partition(units, split, U, clamp=False):
    """Per group g: (u0, u1, main units, tail units, ring pairs)."""
    rows = []
    for g in range(4 * split):
        u0, u1 = wave_range(units, split, g, clamp)
        v = ring_visit(u0, u1, U)
        main = sum(1 for part, _ in v if part != "tail")
        rows.append((u0, u1, main, len(v) - main, main // (2 * U)))
    return rows


def boundary_units(units, split, U, clamp=False):
    """First and last unit of every wave's range and of every ring half
    and tail inside it (sorted, unique)."""
    edges = set()
    for g in range(4 * split):
        u0, u1 = wave_range(units, split, g, clamp)
        v = ring_visit(u0, u1, U)
        for i, (part, u) in enumerate(v):
            first = i == 0 or v[i - 1][0] != part or \
                (part != "tail" and i % U == 0)
            last = i == len(v) - 1 or v[i + 1][0] != part or \
                (part != "tail" and (i + 1) % U == 0)
            if first or last:
                edges.add(u)
    return sorted(edges)


def boundary_ks(K, split, U, unit_k=16, clamp=False):
    """The k positions a needle must probe: the first k of every first
    unit and the last k of every last unit from boundary_units."""
    ks = set()
    for u in boundary_units(K // unit_k, split, U, clamp):
        ks.add(u * unit_k)
        ks.add(u * unit_k + unit_k - 1)
    return sorted(ks)


def needle_batches(ks, M=32):
    """ks in launches of M rows; the last one repeats its final k."""
    out = []
    for i in range(0, len(ks), M):
        chunk = list(ks[i:i + M])
        out.append(chunk + [chunk[-1]] * (M - len(chunk)))
    return out


# --------------------------------------------------------------------------
# case lists (the GPU module runs exactly these)
# --------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    M: int
    N: int
    K: int
    split: int
    seed: int = 0

    @property
    def id(self):
        return f"M{self.M}-N{self.N}-K{self.K}-s{self.split}"


def _cases(table, seeds, n_big=96):
    """Per (K, other split): M = 1 and M = 32 meet every K, at split 1
    and the other split; M = 17 / 31 cycle over N and the splits."""
    out = []
    for i, (K, alt, wide) in enumerate(table):
        nb = n_big if wide else 32
        mid = (17, 31)[i % 2]
        out += [Case(1, 32, K, 1), Case(32, nb, K, alt),
                Case(mid, nb if i % 2 else 32, K, 1 if i % 2 else alt),
                Case(1, nb, K, alt), Case(32, 32, K, 1)]
    assert set(seeds) <= {c.id for c in out}
    return [dataclasses.replace(c, seed=seeds.get(c.id, 0)) for c in out]


# (K, a split other than 1, N = 96 allowed)
BF16_U8_TABLE = [(1024, 2, True), (1040, 8, True), (1536, 3, True),
                 (2032, 2, True), (2048, 4, True), (3056, 3, True),
                 (3072, 8, True), (4096, 2, True), (11008, 4, False)]
# the five K the ring of 12 was sized for, plus what its own edges need:
# 1600 (25 steps per wave: tail 1; split 8 leaves seven waves and one
# k-slice empty) and 4608 (72 per wave: three pairs)
BF16_U12_TABLE = [(1536, 2, True), (1600, 8, True), (2048, 3, True),
                  (3056, 2, True), (3072, 8, True), (4608, 2, True),
                  (11008, 4, False)]
W4_TABLE = [(64, 8, True), (832, 2, True), (2048, 3, True), (2112, 8, True),
            (4032, 2, True), (4096, 3, True), (6144, 2, False)]

# Seeds. Every case uses seed 0 unless listed here: with seed 0 one of the
# mutations below (named after the case) changed no output bit of that
# case, and the listed seed is the first from 0 upwards at which all of
# them do. The usual cause at M = 1 is that one exchanged nibble or
# fragment moves the single affected output by less than half a bf16 ulp
# of a sum over thousands of k; at M = 32 it is a byte whose two nibbles
# are equal (the codes depend on N, K and the seed alone).
BF16_U8_SEEDS = {"M1-N96-K4096-s2": 1}            # middle swap_hi
BF16_U12_SEEDS = {}
W4_SEEDS = {
    "M1-N32-K64-s1": 1, "M1-N32-K832-s1": 7, "M1-N32-K2048-s1": 3,
    "M17-N32-K2048-s3": 1, "M1-N96-K2048-s3": 4, "M32-N32-K2048-s1": 1,
    "M1-N32-K2112-s1": 1, "M32-N32-K2112-s1": 1, "M1-N32-K4032-s1": 10,
    "M17-N32-K4032-s2": 1, "M1-N96-K4032-s2": 3, "M32-N32-K4032-s1": 1,
    "M1-N32-K4096-s1": 1, "M1-N96-K4096-s3": 7, "M32-N32-K4096-s1": 1,
    "M1-N32-K6144-s1": 16, "M1-N32-K6144-s2": 16,   # nibble, bar two: scale
}
GEMM_W4_SEEDS = {(1, 32, 64): 1, (1, 128, 192): 1}  # nibble

BF16_U8_CASES = _cases(BF16_U8_TABLE, BF16_U8_SEEDS)
BF16_U12_CASES = _cases(BF16_U12_TABLE, BF16_U12_SEEDS)
W4_DECODE_CASES = _cases(W4_TABLE, W4_SEEDS)

# gemm_w4: (M, N, K). Every K meets M in {1, 33, 65, 129}; every N meets
# K = 192; M covers the three m-tile variants and their ragged rows.
GEMM_W4_SHAPES = \
    [(M, (32, 96, 128, 160)[(i + j) % 4], K)
     for i, K in enumerate((64, 128, 192, 256, 320, 832))
     for j, M in enumerate((1, 33, 65, 129))] + \
    [(32, 32, 192), (64, 96, 192), (128, 128, 192), (130, 160, 192),
     (32, 160, 64), (64, 128, 320), (128, 96, 832), (130, 32, 256)]
GEMM_W4_CASES = [(M, N, K, GEMM_W4_SEEDS.get((M, N, K), 0))
                 for M, N, K in GEMM_W4_SHAPES]
GEMM_W4_NEEDLE = (129, 160, 320)


def partition_lists():
    """(kernel, K, split, units, U, clamp) of every partition in use."""
    out = []
    for name, cases, U, unit_k, clamp in (
            ("decode_gemm U=8", BF16_U8_CASES, 8, 16, False),
            ("decode_gemm U=12", BF16_U12_CASES, 12, 16, False),
            ("decode_gemm_w4 U=4", W4_DECODE_CASES, 4, 64, True)):
        for K, split in sorted({(c.K, c.split) for c in cases}):
            out.append((name, K, split, K // unit_k, U, clamp))
    return out


def print_partition_table():
    """The table in the GPU module's docstring."""
    last = None
    for name, K, split, units, U, clamp in partition_lists():
        if name != last:
            print(f"{name}  (main + tail units per wave, x count)")
            last = name
        rows, text = partition(units, split, U, clamp), []
        for _, _, main, tail, _ in rows:
            item = "empty" if main + tail == 0 else f"{main}+{tail}"
            if text and text[-1][0] == item:
                text[-1][1] += 1
            else:
                text.append([item, 1])
        line = ", ".join(f"{t} x{n}" if n > 1 else t for t, n in text)
        print(f"  K={K:<6}split={split}  {units:>3} units: {line}")


# --------------------------------------------------------------------------
# swizzle mirrors (from the documented layouts)
# --------------------------------------------------------------------------
LANE = np.arange(64)
ROW = LANE & 31                     # A row / B column / C column of a lane
HI = LANE >> 5
REG = np.arange(16)
# C lane l, register r -> C[row (r&3) + 8 (r>>2) + 4 (l>>5)][col l&31]
C_ROW = (REG[None, :] & 3) + 8 * (REG[None, :] >> 2) + 4 * HI[:, None]
KOFF = HI[:, None] * 8 + np.arange(8)[None, :]        # [64, 8]: k in step


def swizzle_w_mirror(w):
    """ws[nb][s][lane][i] = w[nb*32 + (lane&31)][s*16 + (lane>>5)*8 + i]."""
    N, K = w.shape
    bits = w.view(torch.int16).numpy()
    nb = np.arange(N // 32)[:, None, None, None]
    s = np.arange(K // 16)[None, :, None, None]
    out = bits[nb * 32 + ROW[None, None, :, None],
               s * 16 + KOFF[None, None, :, :]]
    return torch.from_numpy(np.ascontiguousarray(out)).view(torch.bfloat16)


def swizzle_x_mirror(x, pad=0.0):
    """xs[s][lane][i] = x[lane&31][s*16 + (lane>>5)*8 + i] for lane&31 <
    M; every lane with m >= M holds `pad` (the kernel writes zeros)."""
    M, K = x.shape
    full = torch.full((32, K), pad, dtype=torch.bfloat16)
    full[:M] = x
    bits = full.view(torch.int16).numpy()
    s = np.arange(K // 16)[:, None, None]
    out = bits[ROW[None, :, None], s * 16 + KOFF[None, :, :]]
    return torch.from_numpy(np.ascontiguousarray(out)).view(torch.bfloat16)


def w4_frags(wq_swz, sc_swz):
    """A fragments [N/32][K/16][64][8] float64 from decode_gemm_w4.hip's
    stored bytes: dword j of lane l of group g holds, in bits 4i..4i+3,
    nibble i of k-step 4g + j; weight = (nibble - 8) * scale[g][l & 31]."""
    NB, G = wq_swz.shape[:2]
    dw = np.ascontiguousarray(wq_swz.numpy()).view("<u4").reshape(
        NB, G, 64, 4).astype(np.int64)
    nib = (dw[..., None] >> (4 * np.arange(8))) & 0xF   # [NB,G,64,4,8]
    sc = sc_swz.float().numpy().astype(np.float64)      # [NB,G,32]
    a = (nib - 8) * sc[:, :, ROW][..., None, None]
    return a.transpose(0, 1, 3, 2, 4).reshape(NB, G * 4, 64, 8)


# --------------------------------------------------------------------------
# the MFMA and the kernel walk
# --------------------------------------------------------------------------
def mfma_32x32x16(a, b):
    """v_mfma_f32_32x32x16_bf16 on fragments a, b [..., 64, 8] -> the
    lanes' accumulator registers [..., 64, 16]. A lane l -> A[row l&31][k
    (l>>5)*8 + i]; B lane l -> B[k (l>>5)*8 + i][col l&31]; C: C_ROW."""
    A = np.zeros(a.shape[:-2] + (32, 16))
    B = np.zeros(b.shape[:-2] + (16, 32))
    A[..., ROW[:, None], KOFF] = a
    B[..., KOFF, ROW[:, None]] = b
    C = A @ B
    return C[..., C_ROW, ROW[:, None]]


@dataclasses.dataclass
class Mutation:
    """One fault in the walk. nb = None means every n-block."""
    name: str
    nb: int | None = None
    g: int | None = None
    drop: int | None = None          # index into the wave's visit list
    twice: int | None = None
    move: tuple | None = None        # (end 0|1, delta) of the wave's range
    frags: dict | None = None        # {step: (a | None, b | None)}


class Mirror:
    """decode_gemm_kernel (+ combine) over fragment streams. wfrag [N/32]
    [S][64][8] and xfrag [S][64][8] float64 are what lane l loads at step
    s; `unit` k-steps form one partition unit (1: decode_gemm.hip; 4 with
    clamp: the groups of decode_gemm_w4.hip, whose walk is the same)."""

    def __init__(self, wfrag, xfrag, M, N, unit=1, clamp=False):
        self.w, self.x, self.M, self.N = wfrag, xfrag, M, N
        self.unit, self.clamp = unit, clamp
        self.S = xfrag.shape[0]
        assert wfrag.shape[:2] == (N // 32, self.S)
        self.acc_step = mfma_32x32x16(wfrag, xfrag[None])

    def run(self, split, U, mut=None):
        """-> (y bf16 [M,N], slabs fp32 [split,M,N])."""
        M, N, units = self.M, self.N, self.S // self.unit
        slabs = np.zeros((split, M, N), np.float32)
        seen = np.zeros((N // 32, units), np.int64)
        for nb in range(N // 32):
            hit = mut is not None and mut.nb in (None, nb)
            for kslice in range(split):
                red = np.zeros((4, 32, 32), np.float32)
                for wid in range(4):
                    g = kslice * 4 + wid
                    u0, u1 = wave_range(units, split, g, self.clamp)
                    mine = hit and mut.g in (None, g)
                    if mine and mut.move is not None:
                        end, delta = mut.move
                        u0, u1 = (u0 + delta, u1) if end == 0 else \
                            (u0, u1 + delta)
                    visit = [u for _, u in ring_visit(u0, u1, U)]
                    if mine and mut.drop is not None:
                        del visit[mut.drop]
                    if mine and mut.twice is not None:
                        visit.insert(mut.twice, visit[mut.twice])
                    np.add.at(seen[nb], np.array(visit, np.int64), 1)
                    steps = np.array([u * self.unit + j for u in visit
                                      for j in range(self.unit)], np.int64)
                    acc = self.acc_step[nb, steps].sum(axis=0)
                    if hit and mut.frags:
                        for s in steps:
                            if s in mut.frags:
                                a, b = mut.frags[s]
                                a = self.w[nb, s] if a is None else a
                                b = self.x[s] if b is None else b
                                acc += mfma_32x32x16(a, b) - \
                                    self.acc_step[nb, s]
                    acc32 = acc.astype(np.float32)
                    if mut is None:          # fp32 holds every partial sum
                        assert (acc32 == acc).all()
                    red[wid][C_ROW, ROW[:, None]] = acc32
                # thread (em, en): sum of the four waves, n fastest
                tot = ((red[0] + red[1]) + red[2]) + red[3]   # [n][m]
                slabs[kslice, :, nb * 32:nb * 32 + 32] = tot[:, :M].T
        if mut is None:
            assert (seen == 1).all()         # every unit read exactly once
        y = slabs[0].copy()
        for k in range(1, split):
            y = y + slabs[k]
        return torch.from_numpy(y).to(torch.bfloat16), slabs


def mirror_bf16(x, w, pad=0.0):
    M, K = x.shape
    xs = swizzle_x_mirror(x, pad).double().numpy()
    ws = swizzle_w_mirror(w).double().numpy()
    return Mirror(ws, xs, M, w.shape[0])


def mirror_w4(x, q, scales):
    M, K = x.shape
    wq_swz, sc_swz = w4_swizzle_mirror(q, scales)
    xs = swizzle_x_mirror(x).double().numpy()
    m = Mirror(w4_frags(wq_swz, sc_swz), xs, M, q.shape[0], unit=4,
               clamp=True)
    m.wq_swz, m.sc_swz = wq_swz, sc_swz
    return m


def gemm_w4_mirror(x, wfrag):
    """gemm_w4.hip feeds every output k = 0, 16, 32, ... in order through
    the same A fragments: unswizzle them and multiply. float64 [M,N]."""
    NB, S = wfrag.shape[:2]
    W = np.zeros((NB * 32, S * 16))
    nb = np.arange(NB)[:, None, None, None]
    s = np.arange(S)[None, :, None, None]
    W[nb * 32 + ROW[None, None, :, None], s * 16 + KOFF[None, None]] = wfrag
    return x.double().numpy() @ W.T


# --------------------------------------------------------------------------
# mutations at the first, a middle and the last position
# --------------------------------------------------------------------------
POSITIONS = ("first", "middle", "last")


def _pick(seq, pos):
    return seq[{"first": 0, "middle": len(seq) // 2, "last": -1}[pos]]


def _wave_at(mir, split, U, pos):
    """(nb, g, visit length) of the first / a middle / the last wave that
    has work."""
    units = mir.S // mir.unit
    busy = [(g, len(ring_visit(*wave_range(units, split, g, mir.clamp), U)))
            for g in range(4 * split)]
    g, n = _pick([b for b in busy if b[1] > 0], pos)
    return _pick(range(mir.N // 32), pos), g, n


def walk_mutations(mir, split, U, pos):
    """The faults of the walk itself, for either kernel."""
    nb, g, n = _wave_at(mir, split, U, pos)
    i = _pick(range(n), pos)
    units = mir.S // mir.unit
    u0, u1 = wave_range(units, split, g, mir.clamp)
    # a range end that moves without its neighbour following: the first
    # wave reads one unit of the next wave again (or, alone on the whole
    # range, stops one short); a middle wave starts one late; the last
    # one stops one short
    move = {"first": (1, 1 if u1 < units else -1), "middle": (0, 1),
            "last": (1, -1)}[pos]
    return [Mutation("drop", nb, g, drop=i),
            Mutation("twice", nb, g, twice=i),
            Mutation("move", nb, g, move=move)]


def frag_mutations_bf16(mir, pos):
    S, M = mir.S, mir.M
    nb = _pick(range(mir.N // 32), pos)
    s = _pick(range(S), pos)
    sp = min(s, S - 2)                     # x step sp meets w step sp + 1
    r = _pick((0, 13, 31), pos)
    sw = mir.w[nb, s].copy()
    sw[[r, r + 32]] = sw[[r + 32, r]]
    zx = mir.x[s].copy()
    zx[[M - 1, M - 1 + 32]] = 0.0
    return [Mutation("pair", nb, frags={sp: (mir.w[nb, sp + 1], None)}),
            Mutation("swap_hi", nb, frags={s: (sw, None)}),
            Mutation("zero_row", None, frags={s: (None, zx)})]


def frag_mutations_w4(mir, pos):
    """A scale from the next group in one lane; the two nibbles of one
    byte exchanged. With a single group there is no next group: the lane
    takes the next row's scale instead (also a different power of two)."""
    NB, G = mir.wq_swz.shape[:2]
    nb = _pick(range(NB), pos)
    lane = _pick((0, 45, 63), pos)
    g = _pick(range(G - 1), pos) if G > 1 else 0
    sc = mir.sc_swz.clone()
    col = lane & 31
    sc[nb, g, col] = mir.sc_swz[nb, g + 1, col] if G > 1 else \
        mir.sc_swz[nb, g, (col + 1) & 31]
    fr = w4_frags(mir.wq_swz[nb:nb + 1, g:g + 1], sc[nb:nb + 1, g:g + 1])[0]
    scale = {}
    for j in range(4):
        a = mir.w[nb, g * 4 + j].copy()
        a[lane] = fr[j, lane]
        scale[g * 4 + j] = (a, None)
    g, j, byte = _pick(range(G), pos), _pick(range(4), pos), \
        _pick(range(4), pos)
    a = mir.w[nb, g * 4 + j].copy()
    a[lane, [2 * byte, 2 * byte + 1]] = a[lane, [2 * byte + 1, 2 * byte]]
    return [Mutation("scale", nb, frags=scale),
            Mutation("nibble", nb, frags={g * 4 + j: (a, None)})]


def _bits(y):
    return y.contiguous().view(torch.int16)


# --------------------------------------------------------------------------
# tests
# --------------------------------------------------------------------------
def test_ring_partition_covers_each_range_once():
    for name, K, split, units, U, clamp in partition_lists():
        got = []
        for g in range(4 * split):
            u0, u1 = wave_range(units, split, g, clamp)
            v = [u for _, u in ring_visit(u0, u1, U)]
            assert v == list(range(u0, max(u0, u1))), (name, K, split, g)
            got += v
        assert got == list(range(units)), (name, K, split)
    for U in (4, 8, 12):                  # every length, negative included
        for n in range(-40, 80):
            v = ring_visit(5, 5 + n, U)
            assert [u for _, u in v] == list(range(5, 5 + max(n, 0)))
            assert sum(p == "tail" for p, _ in v) == max(n, 0) % (2 * U)


# the edges the lists must reach, per kernel: tails, a tail-only wave, an
# empty wave, an empty k-slice, ring pairs
def _edges(name):
    tails, pairs, flags = set(), set(), set()
    for kname, K, split, units, U, clamp in partition_lists():
        if kname != name:
            continue
        rows = partition(units, split, U, clamp)
        for u0, u1, main, tail, npairs in rows:
            tails.add(tail)
            pairs.add(npairs)
            if main == 0 and tail > 0:
                flags.add("tail-only wave")
            if main + tail == 0:
                flags.add("empty wave")
            if u1 - u0 < 0:
                flags.add("negative range")
        for ks in range(split):
            if all(r[2] + r[3] == 0 for r in rows[4 * ks:4 * ks + 4]):
                flags.add("empty k-slice")
    return tails, pairs, flags


@pytest.mark.parametrize("name,U", [("decode_gemm U=8", 8),
                                    ("decode_gemm U=12", 12),
                                    ("decode_gemm_w4 U=4", 4)])
def test_case_lists_reach_every_edge(name, U):
    tails, pairs, flags = _edges(name)
    assert {0, 1, 2 * U - 1} <= tails, sorted(tails)
    assert {1, 2, 3} <= pairs, sorted(pairs)
    want = {"tail-only wave", "empty wave", "empty k-slice"}
    if U != 4:                            # the w4 kernel clamps its start
        want.add("negative range")
    assert want <= flags, flags


def test_issue_table_partitions():
    """The partitions the case tables were chosen for."""
    def waves(K, split, U, unit_k=16, clamp=False):
        return [(m, t) for _, _, m, t, _ in
                partition(K // unit_k, split, U, clamp)]
    assert waves(1024, 1, 8) == [(16, 0)] * 4
    assert waves(1040, 1, 8) == [(16, 1)] * 3 + [(0, 14)]
    assert waves(1536, 1, 8) == [(16, 8)] * 4
    assert waves(2032, 1, 8) == [(32, 0)] * 3 + [(16, 15)]
    assert waves(3056, 1, 8) == [(48, 0)] * 3 + [(32, 15)]
    assert waves(11008, 4, 8) == [(32, 11)] * 16
    w = waves(1040, 8, 8)
    assert w[:21] == [(0, 3)] * 21 and w[21] == (0, 2)
    assert w[22:] == [(0, 0)] * 10
    assert waves(1536, 1, 12) == [(24, 0)] * 4
    assert waves(2048, 1, 12) == [(24, 8)] * 4
    assert waves(3056, 1, 12) == [(48, 0)] * 3 + [(24, 23)]
    assert waves(11008, 4, 12) == [(24, 19)] * 16
    assert waves(64, 1, 4, 64, True) == [(0, 1)] + [(0, 0)] * 3
    assert waves(2112, 1, 4, 64, True) == [(8, 1)] * 3 + [(0, 6)]
    assert waves(4032, 1, 4, 64, True) == [(16, 0)] * 3 + [(8, 7)]


def test_gemm_w4_case_list_covers_what_it_must():
    ks = {K for _, _, K in GEMM_W4_SHAPES}
    assert ks == {64, 128, 192, 256, 320, 832}
    for K in ks:
        assert {1, 33, 65, 129} <= {M for M, _, k in GEMM_W4_SHAPES if k == K}
    assert {M for M, _, _ in GEMM_W4_SHAPES} == \
        {1, 32, 33, 64, 65, 128, 129, 130}
    assert {N for _, N, K in GEMM_W4_SHAPES if K == 192} == \
        {32, 96, 128, 160}
    assert set(GEMM_W4_SEEDS) <= set(GEMM_W4_SHAPES)
    for table, cases in ((BF16_U8_TABLE, BF16_U8_CASES),
                         (BF16_U12_TABLE, BF16_U12_CASES),
                         (W4_TABLE, W4_DECODE_CASES)):
        for K, alt, _ in table:
            mine = [c for c in cases if c.K == K]
            assert {1, 32} <= {c.M for c in mine}
            assert alt in {c.split for c in mine}
            assert all(c.N in (32, 96) and c.M * c.N <= 160 * 11008
                       for c in mine)
    assert all({1, alt} <= {c.split for c in BF16_U8_CASES if c.K == K}
               for K, alt, _ in BF16_U8_TABLE)


def test_swizzle_mirrors_match_the_host_expressions():
    g = _gen(5)
    w = torch.randn(96, 1040, generator=g).to(torch.bfloat16)
    want = w.view(3, 32, 65, 2, 8).permute(0, 2, 3, 1, 4).contiguous()
    assert torch.equal(_bits(swizzle_w_mirror(w)),
                       _bits(want).view(3, 65, 64, 8))
    x = torch.randn(17, 1040, generator=g).to(torch.bfloat16)
    xs = swizzle_x_mirror(x)
    assert xs.shape == (65, 64, 8)
    assert float(xs[64, 32 + 16, 7]) == float(x[16, 64 * 16 + 15])
    assert bool((xs[:, 17:32] == 0).all()) and bool((xs[:, 49:] == 0).all())
    assert bool((swizzle_x_mirror(x, 1e3)[:, 17:32] == 1e3).all())


def test_needles_read_back_the_probed_column():
    ks = needle_batches(boundary_ks(1040, 1, 8))[0]
    x, w, y = needle_case(32, 32, 1040, ks)
    got, _ = mirror_bf16(x, w).run(1, 8)
    assert torch.equal(_bits(got), _bits(y))
    assert {0, 16 * 17 - 1, 16 * 17, 1039} <= set(boundary_ks(1040, 1, 8))
    x, q, s, y = needle_case_w4(32, 32, 832, list(range(0, 832, 26)))
    got, _ = mirror_w4(x, q, s).run(2, 4)
    assert torch.equal(_bits(got), _bits(y))


def _check_mutations(mir, want, split, U, frag_mutations, case):
    got, slabs = mir.run(split, U)
    assert torch.equal(_bits(got), _bits(want)), case
    for pos in POSITIONS:
        for mut in walk_mutations(mir, split, U, pos) + \
                frag_mutations(mir, pos):
            bad, _ = mir.run(split, U, mut)
            assert not torch.equal(_bits(bad), _bits(want)), \
                (case, pos, mut.name)
    return slabs


@pytest.mark.parametrize("U,cases", [(8, BF16_U8_CASES),
                                     (12, BF16_U12_CASES)],
                         ids=["U8", "U12"])
def test_bf16_mirror_is_exact_and_every_mutation_shows(U, cases):
    for c in cases:
        x, w, y32, y_ref = exact_case_bf16_full(c.M, c.N, c.K, c.seed)
        slabs = _check_mutations(mirror_bf16(x, w), y_ref, c.split, U,
                                 frag_mutations_bf16, c.id)
        assert (slabs.sum(axis=0) == y32.numpy()).all(), c.id


def test_bf16_mirror_ignores_operand_padding():
    for c in BF16_U8_CASES[:3]:
        x, w, y_ref = exact_case_bf16(17, c.N, c.K, c.seed)
        got, _ = mirror_bf16(x, w, pad=1e3).run(c.split, 8)
        assert torch.equal(_bits(got), _bits(y_ref))


def test_w4_mirror_is_exact_and_every_mutation_shows():
    for c in W4_DECODE_CASES:
        x, q, s, _, y_ref = exact_case_w4(c.M, c.N, c.K, c.seed)
        _check_mutations(mirror_w4(x, q, s), y_ref, c.split, 4,
                         frag_mutations_w4, c.id)


def test_gemm_w4_cases_are_exact_and_every_mutation_shows():
    for M, N, K, seed in GEMM_W4_CASES:
        x, q, s, wdq, y_ref = exact_case_w4(M, N, K, seed)
        mir = mirror_w4(x[:1], q, s)          # for its fragments only
        y = torch.from_numpy(gemm_w4_mirror(x, mir.w)).float()
        assert torch.equal(_bits(y.to(torch.bfloat16)), _bits(y_ref))
        for pos in POSITIONS:
            for mut in frag_mutations_w4(mir, pos):
                wf = mir.w.copy()
                for step, (a, _) in mut.frags.items():
                    wf[mut.nb, step] = a
                bad = torch.from_numpy(gemm_w4_mirror(x, wf)).float()
                assert not torch.equal(_bits(bad.to(torch.bfloat16)),
                                       _bits(y_ref)), (M, N, K, pos, mut.name)
