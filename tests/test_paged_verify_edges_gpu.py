"""Verify attention (ops.paged_verify, csrc/attention_verify.hip) at its
edges: every key counted once per query row, the right key in the right row,
and random inputs at a tolerance that notices one lost or extra key.

The structure is that of tests/test_paged_decode_edges_gpu.py, whose helpers
this module imports. The case builders and checkers below are plain CPU
functions; tests/test_paged_verify_edges_cpu.py imports them and proves, on
the reference alone, that each check passes for a right answer and fails for
one wrong key, and that the length lists reach every edge of the kernel's
index arithmetic (row tiles, key splits, waves, the register ring).

A case is q [B, T, Hq, Dh], a plain-layout bf16 K/V pool, a scattered block
table (a random permutation of the pool), seq_lens and q_lens. The device
caches come from it without any append kernel: plain as is, transposed-V by
a permute. Row t of sequence b sees keys [0, ctx + t + 1), ctx = seq_len -
q_len; rows t >= q_len are padding and come back as zeros.

Poison is FINITE (no NaN, no Inf, no block id outside the pool), so a wrong
kernel gives a wrong number, never a fault:
  * every sequence owns one poison block; it sits behind every table entry
    past the sequence's last needed block, and fills the whole table row of
    a q_len = 0 sequence;
  * the slots >= seq_len % 16 of each last live block hold poison rows;
  * a poison K row scores far above any live key for every real query row of
    its (sequence, kv head); its V is 1e3.

Checks (each runs the mixed batch at nsplit 1, 2, 3, 4, 16 and None, and at
nsplit 1 and 4 every sequence alone as B = 1)
  census   q = 0 and V[key p] = e_(p % Dh): out[b, t, h, d] * n_t counts the
           keys p < n_t = ctx + t + 1 with p % Dh == d, so every row of a
           sequence has its own expected vector and one key too many or too
           few at a row's own limit shows on that row. Sums of ones are
           exact in fp32 and only the bf16 store rounds (relative 2^-9), so
           |out * n - count| <= 0.25 while count <= 128. Padding rows and
           rows without keys are exactly 0. (In the 8245-key case at Dh 64
           the census keys are the first Dh and those at positions >= 8191,
           every other V row is 0: that keeps the counts at 2.)
  needle   shapes with G*T <= Dh. Row (t, g) owns head-dim index
           needle_dim(t*G + g): q = 16 e_dim, one key tau <= ctx + t with
           K = 16 e_dim, every other live K entry 0, scale = 1/8. The needle
           scores 32 and holds all but e^-32 of the mass: out is V[tau] to
           one bf16 ulp. The key at ctx + t + 1 (row t+1's own key) carries
           a decoy 32 e_dim on the dims of row (t, .): row t+1 scores 0 on
           it, row t would score 64 if it saw one key too many. Behind the
           last real row's limit lies a dead slot or the poison block.
  random   shapes with G*T <= Dh. randn inputs (q doubled) against float64
           softmax attention per row; metric max|got - ref| / max|ref_row|.
           Each row's first and last visible key hold 15 % of its mass, and
           the key at ctx + t + 1 is built so that row t would score it as
           high as its own last key. The tolerance tau is twice the largest
           metric between the float64 reference and the same reference
           carrying the kernel's rounding points (P -> bf16, out -> bf16;
           q * scale is NOT rounded here, the scale is applied in fp32 after
           the MFMA), over all random cases, measured on the CPU
           (test_paged_verify_edges_cpu.py::test_tau_table recomputes it):

             path         measured    tau
             verify bf16  0.00541     0.01082

           The factor 2 is for fp32 summation order and __expf.
  bits     a sequence run alone equals its rows in the mixed batch
           (torch.equal, nsplit 1 and 4); filling the padding query rows
           with 1e4 changes no output bit; padding rows stay 0.
"""
import dataclasses
import math

import pytest
import torch

from runbooks_amd import ops

from test_paged_decode_edges_gpu import (BS, DEV, NEEDLE_C, NEEDLE_SCALE,
                                         POISON_V, _group_dir, bf16_round,
                                         plain_rows, row_metric)

pytestmark = pytest.mark.gpu

# (G, T, hkv): RT 1; RT 2 in one tile; RT 2 tiled over grid.y
SHAPES = [(1, 1, 2), (1, 8, 2), (3, 2, 2), (4, 4, 2), (2, 8, 2), (16, 1, 1),
          (3, 6, 2), (4, 5, 2), (8, 4, 2), (16, 2, 1),
          (8, 5, 2), (5, 7, 2), (16, 3, 1), (8, 8, 2), (16, 8, 1)]
DHS = (64, 128)
LAYOUTS = ("plain", "vt")
NSPLITS = (1, 2, 3, 4, 16)
ALONE_NSPLITS = (1, 4)

# tolerance of the random test (docstring table)
TAU = 0.01082

NEEDLE_ROUNDS = 4
PAD_FILL = 1e4


def tile_rows(G, T):
    """Query rows per workgroup: 16 (RT 1) or 32 (RT 2)."""
    return 32 if G * T > 16 else 16


def instantiation(dh, layout, G, T):
    return f"<{dh}, {layout}, {tile_rows(G, T) // 16}>"


def length_batches(G, T):
    """Mixed batches of (seq_len, q_len) for a shape. q_len runs through 0,
    1, 2, T-1, T; q_len == seq_len and seq_len = 0 occur; tile block counts
    are 1, 2, 3, 4, 5, 8, 9, 12 and 13; ctx sits at 16k-1, 16k, 16k-T+1 and
    16k-T with q_len = T; where the rows are tiled over grid.y and tile 0
    ends before the last t, ctx + (rows of tile 0) / G == 16k gives the
    later tiles one more block, and small q_len leave them without a row."""
    R = tile_rows(G, T)
    t0 = min((R - 1) // G, T - 1)           # last t of tile 0
    tm = T - 1 if T > 1 else 1
    q2 = min(2, T)
    batches = [
        [(T, T), (0, 0), (9, 0), (1, 1), (15 + T, T), (16 + T, T)],
        [(33, T), (32, T), (13, 1), (64, q2), (79, tm), (48, T)],
        [(128, T), (129, T), (192, tm), (193, T), (143 + T, T), (208, q2)],
    ]
    if G * T > R and t0 < T - 1:
        d = t0 + 1
        batches.append([(16 - d + T, T), (64 - d + T, T), (48 - d + T, d),
                        (50, 1), (128 - d + T, T), (80 - d + T, tm)])
    else:
        batches.append([(17, q2), (31 + T, T), (49, tm), (96, T), (65, 1)])
    return batches


def random_batches(G, T, dh):
    """Batches of the random test: every real row has a prefix of >= 8 keys,
    so that two keys can hold 15 % of its mass each. The first key has to
    meet one score per real row of its kv head; with as many rows as head
    dims (G*T == Dh) that system is square and its solution too long to
    survive bf16, so those two shapes run q_len <= T - 1 here (the census
    and the needle run them at q_len = T)."""
    R = tile_rows(G, T)
    t0 = min((R - 1) // G, T - 1)
    tm = T - 1 if T > 1 else 1
    tf = tm if G * T >= dh else T
    first = [(33, tf), (64, tm), (48 + T, tf), (79 + T, tf), (129, tf),
             (40, 0)]
    second = [(32, tf), (80 - (t0 + 1) + T, tf), (47 + T, min(2, T)),
              (100, 1), (193, tf)]
    return [first, second]


@dataclasses.dataclass
class Case:
    q: torch.Tensor            # [B, T, Hq, Dh] bf16
    k: torch.Tensor            # [NB, Hkv, 16, Dh] bf16, plain layout
    v: torch.Tensor
    bt: torch.Tensor           # [B, MB] int32
    seq_lens: torch.Tensor     # [B] int32
    q_lens: torch.Tensor       # [B] int32
    scale: float
    poison: tuple              # poison block id of every sequence
    G: int
    tau: torch.Tensor = None   # needle tokens [B, T, Hq], -1 = no key
    census_lo: int = 0         # census keys: p < Dh or p >= census_lo

    @property
    def B(self):
        return self.q.shape[0]

    @property
    def T(self):
        return self.q.shape[1]

    def ql(self, b):
        return int(self.q_lens[b])

    def ctx(self, b):
        return int(self.seq_lens[b]) - int(self.q_lens[b])

    def need(self, b):
        """Table entries sequence b reads."""
        return (int(self.seq_lens[b]) + BS - 1) // BS if self.ql(b) else 0


def _mk(dh, G, T, hkv, seqs, seed, scale=None):
    """Zero q and pool; a permuted pool with one poison block per sequence
    behind every table entry that is not needed."""
    gen = torch.Generator().manual_seed(seed)
    B = len(seqs)
    for s, n in seqs:
        assert 0 <= n <= min(s, T), (s, n)
    need = [(s + BS - 1) // BS if n else 0 for s, n in seqs]
    perm = torch.randperm(sum(need) + B, generator=gen).tolist()
    poison, ids = perm[:B], perm[B:]
    MB = max(need) + 2
    bt = torch.empty(B, MB, dtype=torch.int32)
    for b in range(B):
        bt[b] = poison[b]
        for e in range(need[b]):
            bt[b, e] = ids.pop()
    k = torch.zeros(sum(need) + B, hkv, BS, dh, dtype=torch.bfloat16)
    return Case(q=torch.zeros(B, T, hkv * G, dh, dtype=torch.bfloat16),
                k=k, v=torch.zeros_like(k), bt=bt,
                seq_lens=torch.tensor([s for s, _ in seqs], dtype=torch.int32),
                q_lens=torch.tensor([n for _, n in seqs], dtype=torch.int32),
                scale=scale or 1.0 / math.sqrt(dh), poison=tuple(poison), G=G)


def token_index(case, b):
    """(block id, slot, position) of every slot of b's needed blocks."""
    p = torch.arange(case.need(b) * BS)
    return case.bt[b, p // BS].long(), p % BS, p


def poison_dirs(case, score):
    """[B, Hkv, Dh]: the K row on which every real query row of sequence b
    and kv head h scores `score` (min-norm, least squares)."""
    hkv, dh, G = case.k.shape[1], case.k.shape[3], case.G
    dirs = torch.empty(case.B, hkv, dh, dtype=torch.float64)
    for b in range(case.B):
        for h in range(hkv):
            qg = case.q[b, :case.ql(b), h * G:(h + 1) * G].reshape(-1, dh)
            dirs[b, h] = _group_dir(qg, case.scale, score)
    return dirs


def _fill_poison(case, score):
    kd = poison_dirs(case, score).to(torch.bfloat16)
    for b in range(case.B):
        case.k[case.poison[b]] = kd[b][:, None, :]
        case.v[case.poison[b]] = POISON_V
        blk, slot, p = token_index(case, b)
        dead = p >= int(case.seq_lens[b])
        case.k[blk[dead], :, slot[dead]] = kd[b]
        case.v[blk[dead], :, slot[dead]] = POISON_V


# ---- census ---------------------------------------------------------------

def _census_key(p, dh, lo):
    return (p >= lo) | (p < dh)


def census_case(dh, G, T, hkv, seqs, seed=0, lo=0):
    """q = 0; V[p] = e_(p % Dh) on the census keys; K random (it cannot
    matter)."""
    c = _mk(dh, G, T, hkv, seqs, seed)
    c.census_lo = lo
    gen = torch.Generator().manual_seed(seed + 1)
    c.k.copy_(torch.randn(c.k.shape, generator=gen))
    for b in range(c.B):
        blk, slot, p = token_index(c, b)
        onehot = torch.zeros(len(p), dh, dtype=torch.bfloat16)
        on = _census_key(p, dh, lo)
        onehot[torch.arange(len(p))[on], (p % dh)[on]] = 1.0
        c.v[blk, :, slot] = onehot[:, None, :]
    _fill_poison(c, 64.0)
    return c


def census_counts(case):
    """(count [B, T, Dh], n [B, T]) in float64: census keys below each real
    row's limit by residue, and the limit; 0 for padding rows."""
    dh = case.q.shape[3]
    cnt = torch.zeros(case.B, case.T, dh, dtype=torch.float64)
    n = torch.zeros(case.B, case.T, dtype=torch.float64)
    for b in range(case.B):
        ql, ctx = case.ql(b), case.ctx(b)
        if ql == 0:
            continue
        p = torch.arange(ctx + ql)
        onehot = torch.zeros(len(p), dh, dtype=torch.float64)
        on = _census_key(p, dh, case.census_lo)
        onehot[torch.arange(len(p))[on], (p % dh)[on]] = 1.0
        cum = onehot.cumsum(dim=0)
        lim = ctx + 1 + torch.arange(ql)
        cnt[b, :ql] = cum[lim - 1]
        n[b, :ql] = lim.double()
    return cnt, n


def census_row_error(out, case):
    """[B, T]: max |out * n - count| per row; a row without keys (padding
    included) must be exactly 0."""
    cnt, n = census_counts(case)
    o = out.double()
    err = (o * n[:, :, None, None] - cnt[:, :, None, :]).abs().amax((2, 3))
    zero = o.abs().amax((2, 3)) * 1e9
    return torch.where(n == 0, zero, err)


def census_error(out, case):
    return float(census_row_error(out, case).max())


# ---- needle ---------------------------------------------------------------

def needle_dim(rr, dh):
    """Distinct head-dim index per row rr = t*G + g of a kv head (rr < Dh)."""
    return (5 * rr + 2) % dh


def needle_candidates(ctx, t, seq_len):
    """Keys of row t's range [0, ctx + t] worth a needle, most telling
    first: the row's own position, key 0, both sides of the prefix end, the
    key before its own, slots 0 and 15 of the first and last blocks and both
    sides of every split cut (of the row's own and of the sequence's block
    count)."""
    n = ctx + t + 1
    last = (n - 1) // BS
    cand = [ctx + t, 0, ctx - 1, ctx, ctx + t - 1,
            BS - 1, BS * last, BS * last + BS - 1, BS * last - 1]
    for ns in (3, 4, 2, 16):
        for nb in sorted({(n + BS - 1) // BS, (seq_len + BS - 1) // BS}):
            chunk = (nb + ns - 1) // ns
            for j in range(1, ns):
                cand += [BS * j * chunk - 1, BS * j * chunk]
    seen, res = set(), []
    for p in cand:
        if 0 <= p < n and p not in seen:
            seen.add(p)
            res.append(p)
    return res


def needle_case(dh, G, T, hkv, seqs, seed=0, rnd=0, tokens=None):
    """q = 16 e_dim per row, K[tau] = 16 e_dim, decoys 32 e_dim on the key
    behind each row's limit, every other live K = 0, V random. Round `rnd`
    moves every row on through its candidates; `tokens(b, t)` overrides
    them."""
    assert G * T <= dh
    c = _mk(dh, G, T, hkv, seqs, seed, scale=NEEDLE_SCALE)
    gen = torch.Generator().manual_seed(seed + 2)
    c.v.copy_(torch.randn(c.v.shape, generator=gen))
    Hq = hkv * G
    c.tau = torch.full((c.B, T, Hq), -1, dtype=torch.long)
    for b in range(c.B):
        ctx, sl = c.ctx(b), int(c.seq_lens[b])
        for t in range(c.ql(b)):
            cand = tokens(b, t) if tokens else needle_candidates(ctx, t, sl)
            dims = [needle_dim(t * G + g, dh) for g in range(G)]
            for hq in range(Hq):
                p = cand[(3 * rnd + t * Hq + hq + b) % len(cand)]
                assert 0 <= p <= ctx + t
                c.q[b, t, hq, dims[hq % G]] = NEEDLE_C
                c.k[int(c.bt[b, p // BS]), hq // G, p % BS,
                    dims[hq % G]] = NEEDLE_C
                c.tau[b, t, hq] = p
            if t + 1 < c.ql(b):                 # decoy on row t+1's own key
                p = ctx + t + 1
                c.k[int(c.bt[b, p // BS]), :, p % BS, dims] = 2 * NEEDLE_C
    _fill_poison(c, 64.0)
    return c


def needle_expected(case, vref):
    """[B, T, Hq, Dh] float64: V[tau] of every row (0 where it has no key)."""
    B, T, Hq, dh = case.q.shape
    exp = torch.zeros(B, T, Hq, dh, dtype=torch.float64)
    kvh = torch.arange(Hq) // case.G
    for b in range(B):
        rows = plain_rows(vref, case, b)
        tau = case.tau[b]
        exp[b] = rows[tau.clamp(min=0), kvh[None, :]].double()
        exp[b][tau < 0] = 0.0
    return exp


def ulp_error(out, exp):
    """|out - bf16(exp)| in bf16 ulps of the expected value; the other
    keys' e^-32 each shows where V[tau] is tiny, so a ulp counts as 2^-20 at
    least (the decode suite's metric)."""
    exp = bf16_round(exp)
    mag = exp.abs().clamp(min=2.0 ** -13)
    ulp = torch.exp2(torch.floor(torch.log2(mag)) - 7)
    return (out.double() - exp).abs() / ulp


def needle_row_error(out, case, vref):
    """[B, T]: worst ulp error per row; rows without a key exactly 0."""
    err = ulp_error(out, needle_expected(case, vref))
    empty = (case.tau < 0)[..., None].expand_as(err)
    err = torch.where(empty, out.double().abs() * 1e9, err)
    return err.amax((2, 3))


def needle_error(out, case, vref):
    return float(needle_row_error(out, case, vref).max())


# ---- random ---------------------------------------------------------------

HEAVY = math.log(0.15 / 0.70)       # two keys at 15 % each, 70 % the rest


def random_case(dh, G, T, hkv, seqs, seed=0):
    """randn q (doubled), K, V. For every real row the first key and the
    row's own key are moved (min-norm, along the queries) to 15 % of the
    row's mass each; the key at ctx + t is built on the 2G queries of rows
    t-1 and t, so that row t-1 would score it as high as its own last key if
    it saw one key too many."""
    assert G * T <= dh
    c = _mk(dh, G, T, hkv, seqs, seed)
    gen = torch.Generator().manual_seed(seed + 3)
    c.q.copy_(2.0 * torch.randn(c.q.shape, generator=gen))
    c.k.copy_(torch.randn(c.k.shape, generator=gen))
    c.v.copy_(torch.randn(c.v.shape, generator=gen))

    def move(kk, i, qs, want):
        """Key i to the scores `want` on the queries qs; bf16 as stored."""
        have = qs @ kk[i] * c.scale
        knew = kk[i] + torch.linalg.pinv(qs) @ ((want - have) / c.scale)
        kk[i] = knew.to(torch.bfloat16).double()

    for b in range(c.B):
        ql, ctx = c.ql(b), c.ctx(b)
        if ql == 0:
            continue
        assert ctx >= 8, "the random test needs a prefix"
        blk, slot, p = token_index(c, b)
        for h in range(hkv):
            kk = c.k[blk, h, slot].double()              # [16 * need, Dh]
            qs = c.q[b, :ql, h * G:(h + 1) * G].double()  # [ql, G, Dh]
            rest = []
            for t in range(ql):
                pos = ctx + t
                rest.append(torch.logsumexp(
                    kk[1:pos] @ qs[t].T * c.scale, dim=0))
                sel = [t - 1, t] if t else [t]
                move(kk, pos, torch.cat([qs[i] for i in sel]),
                     torch.cat([rest[i] for i in sel]) + HEAVY)
            move(kk, 0, qs.reshape(-1, dh), torch.cat(rest) + HEAVY)
            c.k[blk, h, slot] = kk.to(torch.bfloat16)
    _fill_poison(c, 60.0)
    return c


def plain_random_case(dh, G, T, hkv, seqs, seed=0):
    """randn q, K, V with poison, for the bit-exact invariants (any shape)."""
    c = _mk(dh, G, T, hkv, seqs, seed)
    gen = torch.Generator().manual_seed(seed + 4)
    c.q.copy_(torch.randn(c.q.shape, generator=gen))
    c.k.copy_(torch.randn(c.k.shape, generator=gen))
    c.v.copy_(torch.randn(c.v.shape, generator=gen))
    for b in range(c.B):
        c.q[b, c.ql(b):] = 0
    _fill_poison(c, 40.0)
    return c


def pad_filled(case, value=PAD_FILL):
    """q with every padding row (t >= q_len) set to `value`."""
    q = case.q.clone()
    for b in range(case.B):
        q[b, case.ql(b):] = value
    return q


def ref64(case, kref, vref, shift=0, drop_first=False, rounding=False,
          bt=None):
    """float64 softmax attention per row over plain-layout caches: row t of
    sequence b sees keys [0, ctx + t + 1 + shift), without key 0 if
    `drop_first`, through the table `bt` if given. `rounding` carries the
    kernel's rounding points: P -> bf16 (l from the unrounded P), out ->
    bf16. Rows without a key are 0."""
    B, T, Hq, dh = case.q.shape
    G = case.G
    src = case if bt is None else dataclasses.replace(case, bt=bt)
    out = torch.zeros(B, T, Hq, dh, dtype=torch.float64)
    for b in range(B):
        ql = case.ql(b)
        if ql == 0:
            continue
        lim = case.ctx(b) + 1 + shift + torch.arange(ql)
        P = int(lim.max())
        if P <= 0:
            continue
        kk = plain_rows(kref, src, b)[:P].double().repeat_interleave(G, dim=1)
        vv = plain_rows(vref, src, b)[:P].double().repeat_interleave(G, dim=1)
        qs = case.q[b, :ql].double() * case.scale
        sc = torch.einsum("thd,phd->thp", qs, kk)
        mask = torch.arange(P)[None, :] >= lim[:, None]
        if drop_first:
            mask[:, 0] = True
        sc = sc.masked_fill(mask[:, None, :], float("-inf"))
        mx = sc.amax(dim=-1, keepdim=True)
        p = torch.exp(sc - torch.where(mx == float("-inf"),
                                       torch.zeros_like(mx), mx))
        l = p.sum(dim=-1).clamp(min=1e-300)
        if rounding:
            p = bf16_round(p)
        o = torch.einsum("thp,phd->thd", p, vv) / l[..., None]
        out[b, :ql] = bf16_round(o) if rounding else o
    return out


def host_caches(case, layout):
    """(k, v) in `layout` on the CPU."""
    if layout == "plain":
        return case.k, case.v
    return case.k, case.v.permute(0, 1, 3, 2).contiguous()


def row_case(case, b):
    """The B = 1 view of sequence b (for the checkers)."""
    if b is None:
        return case
    return dataclasses.replace(
        case, q=case.q[b:b + 1], bt=case.bt[b:b + 1],
        seq_lens=case.seq_lens[b:b + 1], q_lens=case.q_lens[b:b + 1],
        poison=case.poison[b:b + 1],
        tau=None if case.tau is None else case.tau[b:b + 1])


# ---- the 8245-key case ----------------------------------------------------

LONG_N = 8192 + 53
# (dh, layout, G, T): <128, vt, RT 2> and <64, plain, RT 1>; hkv = 1
LONG_SHAPES = [(128, "vt", 8, 5), (64, "plain", 4, 4)]
LONG_NSPLITS = (1, 4)
LONG_ROUNDS = 3


def long_census_lo(dh):
    """Census keys everywhere while the counts stay <= 128; else only the
    first Dh keys and those at positions >= 8191."""
    return 0 if (LONG_N + dh - 1) // dh <= 128 else 8191


def long_tokens(T):
    """Needle keys at positions >= 8191 of a (LONG_N, T) sequence."""
    ctx = LONG_N - T

    def tokens(b, t):
        cand = [ctx + t, 8191, 8192, ctx - 1, ctx, 8207, 8208, ctx + t - 1,
                8223, 8224]
        return [p for p in dict.fromkeys(cand) if 8191 <= p <= ctx + t]
    return tokens


# --------------------------------------------------------------------------
# GPU side
# --------------------------------------------------------------------------

def _assert_hip():
    assert ops.has_hip(), "HIP extension not loaded on a GPU box"


class _Dev:
    """A case's tensors on the device, for the whole batch or one row."""

    def __init__(self, case, layout):
        kc, vc = host_caches(case, layout)
        self.case = case
        self.k, self.v = kc.to(DEV), vc.to(DEV)
        self.q, self.bt = case.q.to(DEV), case.bt.to(DEV)
        self.sl, self.ql = case.seq_lens.to(DEV), case.q_lens.to(DEV)

    def run(self, nsplit, row=None, q=None):
        sl = slice(None) if row is None else slice(row, row + 1)
        q = self.q if q is None else q
        return ops.paged_verify(
            q[sl].contiguous(), self.k, self.v, self.bt[sl].contiguous(),
            self.sl[sl].contiguous(), self.ql[sl].contiguous(),
            scale=self.case.scale, nsplit=nsplit).cpu()


def _sweep(dev, check):
    """Run a case mixed (the whole batch) at every split and alone (every
    sequence as B = 1) at nsplit 1 and 4; `check(out, b, nsplit)` asserts
    and returns the error."""
    worst = 0.0
    for nsplit in NSPLITS + (None,):
        worst = max(worst, check(dev.run(nsplit), None, nsplit))
    for nsplit in ALONE_NSPLITS:
        for b in range(dev.case.B):
            worst = max(worst, check(dev.run(nsplit, row=b), b, nsplit))
    return worst


def _params(needle):
    for dh in DHS:
        for layout in LAYOUTS:
            for G, T, hkv in SHAPES:
                if needle and G * T > dh:
                    continue            # a row per head-dim index
                yield pytest.param(dh, layout, G, T, hkv,
                                   id=f"{dh}-{layout}-G{G}-T{T}")


ALL_PARAMS = list(_params(False))
NEEDLE_PARAMS = list(_params(True))


@pytest.mark.parametrize("dh,layout,G,T,hkv", ALL_PARAMS)
def test_census(dh, layout, G, T, hkv):
    """Every key below a row's own limit is counted exactly once, none at
    or past it; padding rows are 0."""
    _assert_hip()
    worst = 0.0
    for i, seqs in enumerate(length_batches(G, T)):
        case = census_case(dh, G, T, hkv, seqs, seed=10 * i + G + T)
        dev = _Dev(case, layout)

        def check(out, b, nsplit):
            err = census_error(out, row_case(case, b))
            assert err <= 0.25, (seqs, b, nsplit, err)
            return err
        worst = max(worst, _sweep(dev, check))
    print("census", instantiation(dh, layout, G, T), f"G{G} T{T}",
          "worst", worst)


@pytest.mark.parametrize("dh,layout,G,T,hkv", NEEDLE_PARAMS)
def test_needle(dh, layout, G, T, hkv):
    """The one key that holds a row's mass reaches the right sequence, row,
    head and dimension, and the key behind the row's limit none of it."""
    _assert_hip()
    worst = 0.0
    for i, seqs in enumerate(length_batches(G, T)):
        for rnd in range(NEEDLE_ROUNDS):
            case = needle_case(dh, G, T, hkv, seqs, seed=10 * i + G + T,
                               rnd=rnd)
            dev = _Dev(case, layout)

            def check(out, b, nsplit):
                err = needle_error(out, row_case(case, b), case.v)
                assert err <= 1.0, (seqs, b, nsplit, rnd, err)
                return err
            worst = max(worst, _sweep(dev, check))
    print("needle", instantiation(dh, layout, G, T), f"G{G} T{T}",
          "worst", worst)


def random_cases(dh, G, T, hkv):
    for i, seqs in enumerate(random_batches(G, T, dh)):
        yield random_case(dh, G, T, hkv, seqs, seed=100 * (i + 1) + G + T + dh)


@pytest.mark.parametrize("dh,layout,G,T,hkv", NEEDLE_PARAMS)
def test_random_against_fp64(dh, layout, G, T, hkv):
    """randn inputs with heavy keys at each row's limit against float64
    attention, at the tolerance of the module docstring's table."""
    _assert_hip()
    worst = 0.0
    for case in random_cases(dh, G, T, hkv):
        dev = _Dev(case, layout)
        ref = ref64(case, case.k, case.v)

        def check(out, b, nsplit):
            r = ref if b is None else ref[b:b + 1]
            m = float(row_metric(out, r).max())
            assert m <= TAU, (b, nsplit, m, TAU)
            for s in range(out.shape[0]):
                ql = int(case.q_lens[s if b is None else b])
                assert not bool(out[s, ql:].any()), (b, nsplit, "padding")
            return m
        worst = max(worst, _sweep(dev, check))
    print("random", instantiation(dh, layout, G, T), f"G{G} T{T}",
          "worst", worst, "tau", TAU)


@pytest.mark.parametrize("dh,layout,G,T,hkv", ALL_PARAMS)
def test_bit_exact_invariants(dh, layout, G, T, hkv):
    """A sequence alone equals its rows in the mixed batch; large values in
    the padding query rows change no output bit; padding rows stay 0."""
    _assert_hip()
    for i, seqs in enumerate(length_batches(G, T)):
        case = plain_random_case(dh, G, T, hkv, seqs, seed=300 + i + G + T)
        dev = _Dev(case, layout)
        qpad = pad_filled(case).to(DEV)
        for nsplit in ALONE_NSPLITS:
            full = dev.run(nsplit)
            assert torch.equal(dev.run(nsplit, q=qpad), full), \
                (seqs, nsplit, "padding rows leaked")
            for b in range(case.B):
                assert not bool(full[b, case.ql(b):].any()), (seqs, nsplit, b)
                alone = dev.run(nsplit, row=b)
                assert torch.equal(alone[0], full[b]), (seqs, nsplit, b)


@pytest.mark.parametrize("dh,layout,G,T", LONG_SHAPES)
def test_more_than_8192_keys_in_one_split(dh, layout, G, T):
    """Past the 512 block-table entries staged in LDS the kernel reads the
    table from global memory (nsplit = 1); at nsplit = 4 every split stages
    its own part of the table, offset by blk_lo. Census and needles at
    positions >= 8191 must hold in both."""
    _assert_hip()
    seqs = [(LONG_N, T)]
    case = census_case(dh, G, T, 1, seqs, seed=77, lo=long_census_lo(dh))
    assert float(census_counts(case)[0].max()) <= 128
    dev = _Dev(case, layout)
    for nsplit in LONG_NSPLITS:
        err = census_error(dev.run(nsplit), case)
        print("long census", instantiation(dh, layout, G, T), nsplit, err)
        assert err <= 0.25, (nsplit, err)
    for rnd in range(LONG_ROUNDS):
        case = needle_case(dh, G, T, 1, seqs, seed=78, rnd=rnd,
                           tokens=long_tokens(T))
        assert int(case.tau.min()) >= 8191
        dev = _Dev(case, layout)
        for nsplit in LONG_NSPLITS:
            err = needle_error(dev.run(nsplit), case, case.v)
            print("long needle", instantiation(dh, layout, G, T), nsplit,
                  rnd, err)
            assert err <= 1.0, (nsplit, rnd, err)
