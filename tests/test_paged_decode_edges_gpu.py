"""Paged decode attention at its edges: every key counted once, the right
key in the right place, and random inputs at a tolerance that notices one
lost key.

The case builders below are plain CPU functions (tests/
test_paged_decode_edges_cpu.py imports them and proves, on the reference
alone, that each check fails for a kernel that loses, repeats or misplaces
one key). A case is q, a plain-layout bf16 K/V pool, a block table, lengths
and optional window starts; each test derives the device caches from it:
plain bf16 as is, transposed-V by a permute, and the two fp8 layouts by
``kv_append_ref`` into a CPU fp8 cache, so no append kernel takes part and
the fp8 reference dequantizes the very bytes the kernel reads.

Every case has
  * a scattered block table (a random permutation of the pool);
  * two poison blocks, and poison rows in the dead slots of live blocks:
    every table entry past the last needed one and every entry wholly before
    the window points to a poison block, the slots >= seq_len % 16 of the
    last live block and the slots < seq_start % 16 of the first hold poison
    rows. A poison K row is built so that every query head of its kv group
    scores far above any live key on it; its V is 1e3. Poison is FINITE on
    purpose: the MFMA kernel multiplies P = 0 by the V tail of the last
    block, recycled cache blocks are always finite in service, and a wrong
    kernel must give a wrong number here, never a fault. No NaN, no Inf, no
    block id outside the pool.

Checks
  census   q = 0 and V[t] = e_(t % Dh): out[d] * n counts the live keys
           with t % Dh == d. Sums of ones are exact in fp32 and only the
           bf16 store rounds (relative 2^-9), so |out * n - count| <= 0.25
           while count <= 128. The fp8 MFMA kernel also rounds P * vscale to
           bf16 (vscale = 1/448 loses 2^-9 there), which halves the count
           this bound covers to 64; the fp8 cases have counts <= 3.
  needle   q_g = 16 e_g, K[tau_g] = 16 e_g, every other live K = 0 and
           scale = 1/8, so the needle scores 32 and holds all but e^-32 of
           the mass: out[b, h] is V[tau] to within one bf16 ulp.
  random   randn inputs (q doubled), first and last live key boosted along
           q to 5-30 % of each row's mass, against float64 softmax
           attention over the gathered live keys. Metric, per (b, h) row:
           max|got - ref| / max|ref_row|. The tolerance tau per path class
           is twice the largest metric between that reference and the same
           reference carrying the kernel's rounding points (q*scale -> bf16
           on the bf16-cache and MFMA paths, P -> bf16 and for fp8
           P*vscale -> bf16 on the MFMA paths, out -> bf16 everywhere),
           over all cases of the random test, measured on the CPU
           (test_paged_decode_edges_cpu.py::test_tau_table recomputes it):

             path class    measured    tau
             scalar bf16   0.0108      0.0216
             MFMA bf16     0.0108      0.0216
             scalar fp8    0.00385     0.0077
             MFMA fp8      0.0106      0.0212

           The factor 2 is for fp32 summation order and __expf. The CPU
           module asserts that dropping the first or the last live key, or
           adding the poison key at position seq_len, moves every case by
           at least 3 tau.
"""
import dataclasses
import math

import pytest
import torch

from runbooks_amd import ops
from runbooks_amd.ops import kvcache

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BS = 16

# every (Dh, G) of the dispatch switch for Dh 64 / 128
INSTANCES = [(128, 1), (128, 2), (128, 4), (128, 8),
             (64, 1), (64, 2), (64, 4), (64, 8), (64, 16)]
NSPLITS = (1, 3, 4, 16)

# tolerance of the random test per path class (docstring table)
TAU = {"scalar_bf16": 0.0216, "mfma_bf16": 0.0216,
       "scalar_fp8": 0.0077, "mfma_fp8": 0.0212}

# Lengths: the issue's fixed list; trip counts 1..5 (both edges) of the
# scalar kernel's strides 4 (head-split bf16, fp8 G>=8), 8 (head-split
# fp8 G=4), 16 (token-split bf16) and 32 (token-split fp8), which also run
# the 2- and 4-deep rings through every "niter mod DEPTH"; 1, 4, 5, 8 and 9
# blocks for the MFMA kernel. One seq_len = 0 row; 5 leaves 11 of 16 splits
# empty.
LENGTH_BATCHES = [
    [1, 15, 16, 17, 31, 32],
    [33, 63, 64, 65, 0, 5],
    [4, 8, 9, 12, 13, 20],
    [24, 25, 48, 49, 80, 96],
    [97, 128, 129, 144, 2, 3],
]
# window starts added in front of those lengths (seq_len = start + length):
# first slot, last slot, block-aligned, one past, two blocks, mid-block
START_CYCLE = [1, 15, 16, 17, 32, 37]

NEEDLE_C = 16.0
NEEDLE_SCALE = 32.0 / (NEEDLE_C * NEEDLE_C)
POISON_V = 1e3


def layouts_for(G):
    """Layouts an instantiation is eligible for (transposed V = MFMA)."""
    return ("plain", "fp8", "vt", "fp8vt") if G >= 4 else ("plain", "fp8")


def path_class(G, layout):
    mfma = layout in ("vt", "fp8vt")
    return ("mfma_" if mfma else "scalar_") + \
        ("fp8" if layout.startswith("fp8") else "bf16")


def hkv_for(G):
    return 2 if G <= 4 else 1


def needle_dim(g):
    """Distinct head-dim index per query head of a group (g < 16)."""
    return (5 * g + 2) % 64


@dataclasses.dataclass
class Case:
    q: torch.Tensor            # [B, Hq, Dh] bf16
    k: torch.Tensor            # [NB, Hkv, 16, Dh] bf16, plain layout
    v: torch.Tensor
    bt: torch.Tensor           # [B, MB] int32
    lens: torch.Tensor         # [B] int32
    starts: torch.Tensor       # [B] int32 or None
    scale: float
    poison: tuple              # the two poison block ids
    G: int
    tau: list = None           # needle tokens, tau[b][h]

    @property
    def B(self):
        return self.q.shape[0]

    def start(self, b):
        return int(self.starts[b]) if self.starts is not None else 0


def poison_target(p, slot, B):
    """Batch row whose queries the K row (poison block p, slot) aims at."""
    return (16 * p + slot) % B


def _layout(lens, starts, hkv, dh, seed):
    """Block table over a permuted pool: live entries get their own blocks,
    every other entry one of the two poison blocks."""
    gen = torch.Generator().manual_seed(seed)
    B = len(lens)
    st = list(starts) if starts is not None else [0] * B
    need = [(n + BS - 1) // BS for n in lens]
    first = [s // BS for s in st]
    nlive = sum(max(0, need[b] - first[b]) for b in range(B))
    perm = torch.randperm(nlive + 2, generator=gen).tolist()
    poison, ids = perm[:2], perm[2:]
    MB = max(need) + 2
    bt = torch.empty(B, MB, dtype=torch.int32)
    for b in range(B):
        for e in range(MB):
            if first[b] <= e < need[b]:
                bt[b, e] = ids.pop()
                continue
            # the slot of this entry next to the live range aims at row b
            # where one of the two blocks can
            slot = 0 if e >= need[b] else BS - 1
            want = [p for p in (0, 1) if poison_target(p, slot, B) == b]
            near = e == need[b] or e == first[b] - 1
            bt[b, e] = poison[want[0] if (want and near) else (b + e) % 2]
    NB = nlive + 2
    k = torch.zeros(NB, hkv, BS, dh, dtype=torch.bfloat16)
    v = torch.zeros_like(k)
    return bt, k, v, tuple(poison)


def token_index(case, b):
    """(block id, slot, token) of every slot of row b's live blocks."""
    n, s = int(case.lens[b]), case.start(b)
    e0, e1 = s // BS, (n + BS - 1) // BS
    if e1 <= e0:
        z = torch.zeros(0, dtype=torch.long)
        return z, z, z
    t = torch.arange(e0 * BS, e1 * BS)
    return case.bt[b, t // BS].long(), t % BS, t


def _fill_poison(case, dirs):
    """dirs [B, Hkv, Dh]: the K row that row b's heads of kv head h all
    score highly on."""
    B = case.B
    kd = dirs.to(torch.bfloat16)
    for p, blk in enumerate(case.poison):
        for slot in range(BS):
            case.k[blk, :, slot] = kd[poison_target(p, slot, B)]
        case.v[blk] = POISON_V
    for b in range(B):
        blk, slot, t = token_index(case, b)
        dead = (t < case.start(b)) | (t >= int(case.lens[b]))
        case.k[blk[dead], :, slot[dead]] = kd[b]
        case.v[blk[dead], :, slot[dead]] = POISON_V


def _group_dir(qg, scale, score):
    """Min-norm K row on which every query of qg [G, Dh] scores `score`."""
    qg = qg.double()
    if not bool(qg.any()):
        return torch.full((qg.shape[1],), 100.0, dtype=torch.float64)
    rhs = torch.full((qg.shape[0],), score / scale, dtype=torch.float64)
    return torch.linalg.pinv(qg) @ rhs


def _poison_dirs(q, hkv, scale, score):
    B, Hq, dh = q.shape
    G = Hq // hkv
    return torch.stack([torch.stack([
        _group_dir(q[b, h * G:(h + 1) * G], scale, score)
        for h in range(hkv)]) for b in range(B)])


def _mk(dh, G, lens, starts, seed, hkv=None):
    hkv = hkv or hkv_for(G)
    bt, k, v, poison = _layout(lens, starts, hkv, dh, seed)
    q = torch.zeros(len(lens), hkv * G, dh, dtype=torch.bfloat16)
    return Case(q=q, k=k, v=v, bt=bt,
                lens=torch.tensor(lens, dtype=torch.int32),
                starts=None if starts is None else
                torch.tensor(starts, dtype=torch.int32),
                scale=1.0 / math.sqrt(dh), poison=poison, G=G)


def with_starts(lengths, rot=0):
    """(seq_lens, starts) for windows of the given lengths."""
    st = [START_CYCLE[(i + rot) % len(START_CYCLE)]
          for i in range(len(lengths))]
    return [s + n for s, n in zip(st, lengths)], st


def census_case(dh, G, lens, starts=None, seed=0, hkv=None):
    """q = 0; V[t] = e_(t % Dh); K random (it cannot matter)."""
    c = _mk(dh, G, lens, starts, seed, hkv)
    gen = torch.Generator().manual_seed(seed + 1)
    c.k.copy_(torch.randn(c.k.shape, generator=gen))
    for b in range(c.B):
        blk, slot, t = token_index(c, b)
        onehot = torch.zeros(len(t), dh, dtype=torch.bfloat16)
        onehot[torch.arange(len(t)), t % dh] = 1.0
        c.v[blk, :, slot] = onehot[:, None, :]
    _fill_poison(c, _poison_dirs(c.q, c.k.shape[1], c.scale, 64.0))
    return c


def census_counts(case):
    """[B, Dh] float64: live keys per residue, and the window lengths."""
    dh = case.q.shape[2]
    cnt = torch.zeros(case.B, dh, dtype=torch.float64)
    for b in range(case.B):
        t = torch.arange(case.start(b), int(case.lens[b]))
        cnt[b] = torch.bincount(t % dh, minlength=dh).double()
    return cnt


def census_error(out, case):
    """max |out * n - count|; a row with no live key must be exactly 0."""
    cnt = census_counts(case)
    n = cnt.sum(dim=1)
    got = out.double() * n[:, None, None]
    err = (got - cnt[:, None, :]).abs()
    empty = n == 0
    if bool(empty.any()):
        err[empty] = out.double()[empty].abs() * 1e9
    return float(err.max())


def needle_candidates(n, s):
    """Tokens of the window [s, n) worth a needle, most telling first:
    the ends, both sides of every split cut, slots 0 and 15 of the first
    and last blocks, the last iteration of each wave of the scalar kernel
    (4- and 8-token wave passes) and the last block of each wave of the
    MFMA kernel."""
    ln = n - s
    cand = [s, n - 1]
    for ns in (3, 4):
        chunk = (ln + ns - 1) // ns
        for j in range(1, ns):
            cand += [s + j * chunk - 1, s + j * chunk]
    for e in ((n - 1) // BS, s // BS, s // BS + 1):
        cand += [e * BS - 1, e * BS, e * BS + BS - 1]
    cand += [n - 1 - 4 * j for j in range(1, 4)]
    cand += [n - 1 - 8 * j for j in range(1, 4)]
    cand += [n - 1 - 16 * j for j in range(1, 4)]
    chunk = (ln + 15) // 16
    for j in range(1, 16):
        cand += [s + j * chunk - 1, s + j * chunk]
    seen, res = set(), []
    for t in cand:
        if s <= t < n and t not in seen:
            seen.add(t)
            res.append(t)
    return res


def needle_case(dh, G, lens, starts=None, seed=0, rnd=0, tokens=None,
                hkv=None):
    """q_g = c e_g, K[tau_g] = c e_g, every other live K = 0, V random.
    Round `rnd` moves every head on to its next candidate token; heads
    share a token only where the window has fewer tokens than heads.
    `tokens` (a list per sequence) overrides the candidates."""
    c = _mk(dh, G, lens, starts, seed, hkv)
    c.scale = NEEDLE_SCALE
    hkv = c.k.shape[1]
    gen = torch.Generator().manual_seed(seed + 2)
    c.v.copy_(torch.randn(c.v.shape, generator=gen))
    for h in range(hkv * G):
        c.q[:, h, needle_dim(h % G)] = NEEDLE_C
    c.tau = []
    for b in range(c.B):
        n, s = int(c.lens[b]), c.start(b)
        cand = tokens[b] if tokens is not None else needle_candidates(n, s)
        row = []
        for h in range(hkv * G):
            if not cand:
                row.append(-1)
                continue
            t = cand[(rnd * hkv * G + h + 3 * b) % len(cand)]
            c.k[int(c.bt[b, t // BS]), h // G, t % BS,
                needle_dim(h % G)] = NEEDLE_C
            row.append(t)
        c.tau.append(row)
    _fill_poison(c, _poison_dirs(c.q, hkv, c.scale, 64.0))
    return c


def plain_rows(cache, case, b):
    """[16 * entries, Hkv, Dh]: row b's virtual token axis gathered from a
    plain-layout cache through its block table."""
    blocks = case.bt[b].long()
    x = cache[blocks]                       # [MB, Hkv, 16, Dh]
    return x.transpose(1, 2).reshape(-1, x.shape[1], x.shape[3])


def needle_expected(case, vref):
    """[B, Hq, Dh] float64: V[tau] of every head (0 where no live key)."""
    B, Hq, dh = case.q.shape
    exp = torch.zeros(B, Hq, dh, dtype=torch.float64)
    for b in range(B):
        rows = plain_rows(vref, case, b)
        for h in range(Hq):
            if case.tau[b][h] >= 0:
                exp[b, h] = rows[case.tau[b][h], h // case.G].double()
    return exp


def bf16_round(x):
    return x.float().to(torch.bfloat16).double()


def needle_error(out, case, vref):
    """max |out - bf16(V[tau])| in bf16 ulps of the expected value. The
    other keys' e^-32 each (< 1e-9 of the mass in all) shows where V[tau]
    is 0 or tiny, as fp8 rows have it, so a ulp counts as 2^-20 at least."""
    exp = bf16_round(needle_expected(case, vref))
    mag = exp.abs().clamp(min=2.0 ** -13)
    ulp = torch.exp2(torch.floor(torch.log2(mag)) - 7)
    err = (out.double() - exp).abs() / ulp
    empty = torch.tensor(case.tau) < 0      # no live key: exactly 0
    err[empty] = out.double()[empty].abs() * 1e9
    return float(err.max())


def random_case(dh, G, lens, starts=None, seed=0):
    """randn q (doubled), K, V; the first and the last live key moved along
    the group's queries so that each holds ~15 % of every row's mass."""
    c = _mk(dh, G, lens, starts, seed)
    hkv = c.k.shape[1]
    gen = torch.Generator().manual_seed(seed + 3)
    c.q.copy_(2.0 * torch.randn(c.q.shape, generator=gen))
    c.k.copy_(torch.randn(c.k.shape, generator=gen))
    c.v.copy_(torch.randn(c.v.shape, generator=gen))
    for b in range(c.B):
        n, s = int(c.lens[b]), c.start(b)
        assert n - s >= 8, "the random test needs a few live keys"
        blk, slot, t = token_index(c, b)
        live = (t >= s) & (t < n)
        blk, slot = blk[live], slot[live]
        for h in range(hkv):
            qg = c.q[b, h * G:(h + 1) * G].double()          # [G, Dh]
            kk = c.k[blk, h, slot].double()                  # [n - s, Dh]
            sc = kk @ qg.T * c.scale                         # [n - s, G]
            rest = torch.logsumexp(sc[1:-1], dim=0)
            want = rest + math.log(0.15 / 0.70)
            pin = torch.linalg.pinv(qg)
            for i in (0, -1):
                knew = kk[i] + pin @ ((want - sc[i]) / c.scale)
                c.k[blk[i], h, slot[i]] = knew.to(torch.bfloat16)
    _fill_poison(c, _poison_dirs(c.q, hkv, c.scale, 60.0))
    return c


def ref64(case, kref, vref, lens=None, starts=None, drop=None,
          rounding=None, vscale=None):
    """float64 softmax attention over the gathered live keys of plain-layout
    caches (bf16, or dequantized fp8). `drop` removes one live key by its
    index in the window (0 first, -1 last). `rounding` in {"scalar_bf16",
    "mfma_bf16", "scalar_fp8", "mfma_fp8"} carries the kernel's rounding
    points; "mfma_fp8" needs the per-token V scales `vscale`
    [NB, Hkv, 16]."""
    B, Hq, dh = case.q.shape
    G = case.G
    out = torch.zeros(B, Hq, dh, dtype=torch.float64)
    lens = case.lens if lens is None else lens
    for b in range(B):
        n = int(lens[b])
        s = int(starts[b]) if starts is not None else case.start(b)
        if n <= s:
            continue
        keep = torch.arange(s, n)
        if drop is not None:
            i = drop % len(keep)
            keep = torch.cat([keep[:i], keep[i + 1:]])
        kk = plain_rows(kref, case, b)[keep].double()     # [m, Hkv, Dh]
        vv = plain_rows(vref, case, b)[keep].double()
        qs = case.q[b].double() * case.scale
        if rounding in ("scalar_bf16", "mfma_bf16", "mfma_fp8"):
            qs = bf16_round(case.q[b].float() * case.scale)
        kk = kk.repeat_interleave(G, dim=1)               # [m, Hq, Dh]
        vv = vv.repeat_interleave(G, dim=1)
        sc = torch.einsum("mhd,hd->mh", kk, qs)
        p = torch.exp(sc - sc.max(dim=0).values)
        l = p.sum(dim=0)
        if rounding == "mfma_bf16":
            p = bf16_round(p)
        elif rounding == "mfma_fp8":
            vs = vscale[case.bt[b].long()].transpose(1, 2).reshape(
                -1, vscale.shape[1])[keep].double()
            vs = vs.repeat_interleave(G, dim=1)           # [m, Hq]
            p = bf16_round(p * vs) / vs
        o = torch.einsum("mh,mhd->hd", p, vv) / l[:, None]
        out[b] = bf16_round(o) if rounding else o
    return out


def row_metric(got, ref):
    """[B, Hq]: max|got - ref| / max|ref_row|."""
    den = ref.abs().amax(dim=-1).clamp(min=1e-30)
    return (got.double() - ref).abs().amax(dim=-1) / den


def host_caches(case, layout):
    """(k, v) in `layout` on the CPU, plus the plain-layout float values the
    kernel will read (kref, vref) and, for fp8, the V scales."""
    if layout == "plain":
        return case.k, case.v, case.k, case.v, None
    if layout == "vt":
        return (case.k, case.v.permute(0, 1, 3, 2).contiguous(),
                case.k, case.v, None)
    NB, hkv, _, dh = case.k.shape
    vt = layout == "fp8vt"
    kc, vc = kvcache.alloc_kv_cache(NB, hkv, dh, "cpu", fp8=True,
                                    v_transposed=vt)
    kvcache.kv_append_ref(
        case.k.transpose(1, 2).reshape(NB * BS, hkv, dh),
        case.v.transpose(1, 2).reshape(NB * BS, hkv, dh),
        kc, vc, torch.arange(NB * BS, dtype=torch.int32))
    kref = kvcache.fp8_dequant_cache_ref(kc)
    vref = kvcache.fp8_dequant_cache_ref(vc)
    if vt:
        vref = vref.permute(0, 1, 3, 2).contiguous()
        vs = vc[:, :, dh:, :].reshape(NB, hkv, -1).contiguous().view(
            torch.float32)
    else:
        vs = vc[..., dh:dh + 4].contiguous().view(torch.float32)[..., 0]
    return kc, vc, kref, vref, vs


# --------------------------------------------------------------------------
# GPU side
# --------------------------------------------------------------------------

def _assert_hip():
    assert ops.has_hip(), "HIP extension not loaded on a GPU box"


class _Dev:
    """A case's tensors on the device, for the whole batch or one row."""

    def __init__(self, case, layout):
        kc, vc, self.kref, self.vref, self.vs = host_caches(case, layout)
        self.case = case
        self.k, self.v = kc.to(DEV), vc.to(DEV)
        self.q, self.bt = case.q.to(DEV), case.bt.to(DEV)
        self.lens = case.lens.to(DEV)
        self.starts = None if case.starts is None else case.starts.to(DEV)

    def args(self, row=None):
        sl = slice(None) if row is None else slice(row, row + 1)
        st = None if self.starts is None else self.starts[sl].contiguous()
        return (self.q[sl].contiguous(), self.k, self.v,
                self.bt[sl].contiguous(), self.lens[sl].contiguous()), st

    def run(self, nsplit, row=None):
        a, st = self.args(row)
        return ops.paged_decode(*a, scale=self.case.scale, nsplit=nsplit,
                                seq_starts=st).cpu()


def _grid_batches(windowed):
    for i, lengths in enumerate(LENGTH_BATCHES):
        if windowed:
            yield with_starts(lengths, rot=i)
        else:
            yield lengths, None


def _sweep(dev, check, what):
    """Run a case mixed (the whole batch) and alone (every row as B = 1)
    at every split; `check(out, rows)` returns the error to print and
    assert on."""
    worst = 0.0
    for nsplit in NSPLITS + (None,):
        worst = max(worst, check(dev.run(nsplit), None, nsplit))
        if nsplit is None:
            continue
        for b in range(dev.case.B):
            worst = max(worst, check(dev.run(nsplit, row=b), b, nsplit))
    print(what, "worst", worst)


def _row_case(case, b):
    """The B = 1 view of row b (for the checkers)."""
    if b is None:
        return case
    return dataclasses.replace(
        case, q=case.q[b:b + 1], bt=case.bt[b:b + 1],
        lens=case.lens[b:b + 1],
        starts=None if case.starts is None else case.starts[b:b + 1],
        tau=None if case.tau is None else case.tau[b:b + 1])


INST_LAYOUTS = [(dh, G, lay) for dh, G in INSTANCES for lay in layouts_for(G)]


@pytest.mark.parametrize("windowed", [False, True])
@pytest.mark.parametrize("dh,G,layout", INST_LAYOUTS)
def test_census(dh, G, layout, windowed):
    """Every live key is counted exactly once, none outside the window."""
    _assert_hip()
    for i, (lens, starts) in enumerate(_grid_batches(windowed)):
        case = census_case(dh, G, lens, starts, seed=10 * i + G)
        dev = _Dev(case, layout)

        def check(out, b, nsplit):
            err = census_error(out, _row_case(case, b))
            assert err <= 0.25, (lens, starts, b, nsplit, err)
            return err
        _sweep(dev, check, f"census {dh} {G} {layout} {lens}")


NEEDLE_ROUNDS = {"plain": 8, "vt": 8, "fp8": 4, "fp8vt": 4}


@pytest.mark.parametrize("windowed", [False, True])
@pytest.mark.parametrize("dh,G,layout", INST_LAYOUTS)
def test_needle(dh, G, layout, windowed):
    """The one key that holds the mass reaches the right batch row, head
    and dimension: out[b, h] is V[tau] to one bf16 ulp."""
    _assert_hip()
    for i, (lens, starts) in enumerate(_grid_batches(windowed)):
        for rnd in range(NEEDLE_ROUNDS[layout]):
            case = needle_case(dh, G, lens, starts, seed=10 * i + G, rnd=rnd)
            dev = _Dev(case, layout)

            def check(out, b, nsplit):
                err = needle_error(out, _row_case(case, b), dev.vref)
                assert err <= 1.0, (lens, starts, b, nsplit, rnd, err)
                return err
            _sweep(dev, check, f"needle {dh} {G} {layout} {lens} r{rnd}")


LONG_N = 8192 + 16 * 3 + 5
LONG_NEEDLES = [8192, LONG_N - 1, 8207, 8208, 8191, 8224, 8239, 8240]


@pytest.mark.parametrize("G,layout", [(1, "plain"), (4, "plain"), (4, "vt")])
def test_more_than_8192_keys_in_one_split(G, layout):
    """Past the 512 block-table entries staged in LDS the kernels read the
    table from global memory (nsplit = 1); with nsplit = 4 nothing leaves
    LDS. Census and needles at tokens >= 8192 must hold in both."""
    _assert_hip()
    dh = 128
    case = census_case(dh, G, [LONG_N], None, seed=77, hkv=1)
    assert float(census_counts(case).max()) <= 128
    dev = _Dev(case, layout)
    for nsplit in (1, 4):
        err = census_error(dev.run(nsplit), case)
        print("long census", G, layout, nsplit, err)
        assert err <= 0.25, (nsplit, err)
    for rnd in range(len(LONG_NEEDLES) // G):
        case = needle_case(dh, G, [LONG_N], None, seed=78, rnd=rnd,
                           tokens=[LONG_NEEDLES], hkv=1)
        assert all(t >= 8191 for t in case.tau[0])
        dev = _Dev(case, layout)
        for nsplit in (1, 4):
            err = needle_error(dev.run(nsplit), case, dev.vref)
            print("long needle", G, layout, nsplit, rnd, case.tau, err)
            assert err <= 1.0, (nsplit, rnd, err)


# The random test's batches. A sequence whose length is a multiple of 16,
# or whose window starts on one, sits in a batch row that a poison block's
# slot 0 / slot 15 aims at (poison_target), so the key next to its live
# range is decisive for it.
RANDOM_LENS6 = [64, 17, 33, 65, 144, 129]
RANDOM_WIN6 = ([64, 17, 33, 65, 144, 129], [1, 32, 17, 16, 37, 5])
RANDOM_LENS4 = [64, 33, 65, 129]
RANDOM_WIN4 = ([64, 33, 65, 129], [1, 17, 37, 16])


def random_cases(dh, G):
    """The two mixed batches of the random test: whole sequences, and
    windows. B * Hq <= 64."""
    if G == 16:
        lens, (wl, ws) = RANDOM_LENS4, RANDOM_WIN4
    else:
        lens, (wl, ws) = RANDOM_LENS6, RANDOM_WIN6
    yield random_case(dh, G, lens, None, seed=100 + G + dh)
    yield random_case(dh, G, [s + n for s, n in zip(ws, wl)], ws,
                      seed=200 + G + dh)


@pytest.mark.parametrize("dh,G,layout", INST_LAYOUTS)
def test_random_against_fp64(dh, G, layout):
    """randn inputs with two heavy keys against float64 attention, at the
    tolerance of the module docstring's table."""
    _assert_hip()
    tau = TAU[path_class(G, layout)]
    for case in random_cases(dh, G):
        dev = _Dev(case, layout)
        ref = ref64(case, dev.kref, dev.vref)
        for nsplit in NSPLITS + (None,):
            m = float(row_metric(dev.run(nsplit), ref).max())
            print("random", dh, G, layout, nsplit, "metric", m, "tau", tau)
            assert m <= tau, (nsplit, m, tau)


@pytest.mark.parametrize("dh,G,layout", INST_LAYOUTS)
def test_batch_independence(dh, G, layout):
    """A row of the mixed batch equals, bit for bit, the same sequence run
    alone on the same cache."""
    _assert_hip()
    for case in random_cases(dh, G):
        dev = _Dev(case, layout)
        for nsplit in (1, 4):
            full = dev.run(nsplit)
            for b in range(case.B):
                alone = dev.run(nsplit, row=b)
                assert torch.equal(alone[0], full[b]), (nsplit, b)


@pytest.mark.parametrize("dh,G,layout", INST_LAYOUTS)
def test_operand_emit(dh, G, layout):
    """The fused o_proj operand is decode_swizzle_x(out) on rows < B where
    the wrapper returns one (token-split and head-split epilogues, MFMA
    epilogue, combine kernel), and None for Dh 64 without a split."""
    _assert_hip()
    case = next(random_cases(dh, G))
    dev = _Dev(case, layout)
    B, Hq, _ = case.q.shape
    K = Hq * dh
    for nsplit in (1, 3, 4):
        a, st = dev.args()
        out, swz = ops.paged_decode_with_operand(
            *a, scale=case.scale, nsplit=nsplit, seq_starts=st)
        assert torch.equal(out.cpu(), dev.run(nsplit)), nsplit
        if dh == 64 and nsplit <= 1:
            assert swz is None
            continue
        assert swz is not None, nsplit
        ref = ops.ext().decode_swizzle_x(out.reshape(B, K).contiguous())
        s_v = swz.view(K // 16, 2, 32, 8)[:, :, :B]
        r_v = ref.view(K // 16, 2, 32, 8)[:, :, :B]
        assert torch.equal(s_v, r_v), nsplit
