"""CPU proof that tests/test_paged_verify_edges_gpu.py would notice a subtly
wrong verify kernel, without ever running one.

  * A pure-Python model of the kernel's index arithmetic (lengths, row
    tiles, key splits, blocks per wave) asserts that the length lists reach
    every edge the GPU module's docstring names.
  * For every case its builders make, the fp32 reference
    (ops.paged_verify_ref) passes the very checkers the GPU tests use, in
    both cache layouts.
  * The float64 reference fed ONE wrong key -- every row's limit moved by
    +1 (for the last row that is the poison key at seq_len) or by -1, the
    first key dropped, a table entry pointing into another sequence's
    block -- fails them, at every real row.
  * The random test's tolerance is recomputed here.
"""
import dataclasses

import pytest
import torch

from runbooks_amd import ops

import test_paged_verify_edges_gpu as V

BS = V.BS
SHAPE_IDS = [f"G{G}-T{T}" for G, T, _ in V.SHAPES]


# --------------------------------------------------------------------------
# index model of attention_verify.hip: the "lengths" prologue and the wave
# loop. Not a numeric simulator.
# --------------------------------------------------------------------------

def verify_index(seq_len, q_len, G, T, nsplit, max_blocks):
    """One record per (row tile, key split) of a (sequence, kv head)."""
    R = V.tile_rows(G, T)
    ntile = (G * T + R - 1) // R
    seq_len = min(max(seq_len, 0), max_blocks * BS)
    q_len = min(min(max(q_len, 0), T), seq_len)
    ctx = seq_len - q_len
    if q_len == 0:
        seq_len = 0
    recs = []
    for tile in range(ntile):
        rbase = tile * R
        t_lo = rbase // G
        t_hi = min((rbase + R - 1) // G, T - 1, q_len - 1)
        kmax = ctx + t_hi + 1 if t_hi >= t_lo else 0
        nblk = (kmax + BS - 1) // BS
        chunk = (nblk + nsplit - 1) // nsplit
        for split in range(nsplit):
            blk_lo = split * chunk
            blk_hi = min(nblk, blk_lo + chunk) - 1
            waves = [len(range(blk_lo + w, blk_hi + 1, 4)) for w in range(4)]
            # real rows of the tile and the keys each has in this split
            rows = [rr // G for rr in range(rbase, min(rbase + R, G * T))
                    if rr // G < q_len]
            keys = [max(0, min(ctx + t + 1, (blk_hi + 1) * BS) - blk_lo * BS)
                    for t in rows]
            recs.append(dict(
                tile=tile, split=split, ntile=ntile, ctx=ctx, t_lo=t_lo,
                t_hi=t_hi, kmax=kmax, nblk=nblk, chunk=chunk, blk_lo=blk_lo,
                blk_hi=blk_hi, nb=max(0, blk_hi - blk_lo + 1), waves=waves,
                row_keys=keys))
    return recs


def _batch_records(G, T, seqs, nsplit):
    mb = max((s + BS - 1) // BS if n else 0 for s, n in seqs) + 2
    for s, n in seqs:
        yield (s, n), verify_index(s, n, G, T, nsplit, mb)


def test_index_model_matches_the_issue_example():
    """seq_len 33, q_len 8, nsplit 3: the last split holds a key for row 7
    only; 5 blocks at nsplit 4 split 2, 2, 1, 0."""
    recs = verify_index(33, 8, 2, 8, 3, 5)
    assert [r["nb"] for r in recs] == [1, 1, 1]
    assert recs[2]["row_keys"] == [0] * 14 + [1, 1]
    recs = verify_index(79, 4, 4, 4, 4, 7)
    assert [r["nb"] for r in recs] == [2, 2, 1, 0]
    # (8, 5): tile 0 is t 0..3, tile 1 is t 4; ctx + 4 == 16 k
    recs = verify_index(64 - 4 + 5, 5, 8, 5, 1, 7)
    assert [(r["t_lo"], r["t_hi"], r["nblk"]) for r in recs] == \
        [(0, 3, 4), (4, 4, 5)]
    # (5, 7): the tile cut lies inside t = 6
    recs = verify_index(40, 7, 5, 7, 1, 5)
    assert [(r["t_lo"], r["t_hi"]) for r in recs] == [(0, 6), (6, 6)]


def test_shape_list_reaches_every_instantiation():
    inst = {V.instantiation(dh, lay, G, T)
            for dh in V.DHS for lay in V.LAYOUTS for G, T, _ in V.SHAPES}
    assert len(inst) == 8
    shapes = {(G, T): hkv for G, T, hkv in V.SHAPES}
    assert set(shapes) >= {
        (1, 1), (1, 8), (3, 2), (4, 4), (2, 8), (16, 1), (3, 6), (4, 5),
        (8, 4), (16, 2), (8, 5), (5, 7), (16, 3), (8, 8), (16, 8)}
    for G, T in ((5, 7), (8, 5), (3, 6), (4, 4)):
        assert shapes[(G, T)] == 2
    assert all(hkv == 1 for (G, _), hkv in shapes.items() if G == 16)
    # needle and random leave out only shapes with more rows than Dh
    left = {(p.values[0], p.values[2], p.values[3]) for p in V.ALL_PARAMS} - \
        {(p.values[0], p.values[2], p.values[3]) for p in V.NEEDLE_PARAMS}
    assert left == {(64, 16, 8)}
    assert all(G * T > dh for dh, G, T in left)
    assert (128, "vt", 8, 5) in V.LONG_SHAPES
    assert (64, "plain", 4, 4) in V.LONG_SHAPES


@pytest.mark.parametrize("G,T,hkv", V.SHAPES, ids=SHAPE_IDS)
def test_lengths_reach_every_edge(G, T, hkv):
    """The length batches of a shape, run through the index model."""
    batches = V.length_batches(G, T)
    assert all(4 <= len(b) <= 6 for b in batches)
    seqs = [x for b in batches for x in b]
    assert {n for _, n in seqs} >= {n for n in (0, 1, 2, T - 1, T)
                                    if 0 <= n <= T}
    assert any(s == n > 0 for s, n in seqs)         # no prefix
    assert any(s == 0 for s, n in seqs)
    assert any(s > 0 and n == 0 for s, n in seqs)   # poison-only table row
    # new tokens straddle a block edge: ctx at 16k-1, 16k, 16k-T+1, 16k-T
    ctxs = {s - n for s, n in seqs if n == T}
    for off in (-1, 0, 1 - T, -T):
        assert any(c > 0 and (c - off) % BS == 0 and c - off >= BS
                   for c in ctxs), off

    R = V.tile_rows(G, T)
    t0 = min((R - 1) // G, T - 1)
    per_split, wave_blocks, facts = set(), set(), set()
    for nsplit in V.NSPLITS:
        for b in batches:
            for (s, n), recs in _batch_records(G, T, b, nsplit):
                for r in recs:
                    per_split.add(r["nb"])
                    wave_blocks |= set(r["waves"])
                    if r["nb"] and r["blk_lo"] > 0:
                        facts.add("offset table")
                    if r["nb"] and 0 in r["row_keys"] and any(r["row_keys"]):
                        facts.add("split without keys for some row")
                    if r["tile"] and r["t_hi"] < r["t_lo"] and n > 0:
                        facts.add("later tile without a row")
                    if r["tile"] and r["nblk"] == recs[0]["nblk"] + 1:
                        facts.add("later tile needs one more block")
                    if nsplit == 1:
                        facts.add(("nblk", r["nblk"]))
                for tile in range(recs[0]["ntile"]):
                    nbs = [r["nb"] for r in recs if r["tile"] == tile]
                    if nsplit == 4 and nbs == [2, 2, 1, 0]:
                        facts.add("empty trailing split")
                    if nsplit == 16 and sum(nbs) and nbs.count(0) >= 11:
                        facts.add("mostly empty splits")
    # 0..3 (and 4) blocks per wave: the ring ends on either slot
    assert {0, 1, 2, 3, 4} <= wave_blocks
    assert {1, 2, 3, 4, 5, 8, 9, 12, 13} <= per_split
    assert {("nblk", k) for k in (1, 2, 3, 4, 5, 8, 9, 12, 13)} <= facts
    assert {"offset table", "empty trailing split",
            "mostly empty splits"} <= facts
    if T >= 2:
        assert "split without keys for some row" in facts
    if G * T > R:
        assert "later tile without a row" in facts
        if t0 < T - 1:
            assert "later tile needs one more block" in facts
    # the random batches: a prefix for every real row, tiles included
    for dh in V.DHS:
        for b in V.random_batches(G, T, dh):
            assert 4 <= len(b) <= 6
            assert all(n == 0 or s - n >= 8 for s, n in b)
            assert all(n * G < dh or G * T > dh for s, n in b)


def test_long_case_leaves_the_staged_table():
    """516 blocks: one split reads entries 512.. from global memory; four
    splits stage 129 entries each at a nonzero offset."""
    for dh, layout, G, T in V.LONG_SHAPES:
        one = verify_index(V.LONG_N, T, G, T, 1, 518)
        assert all(r["nb"] > 512 for r in one)
        four = verify_index(V.LONG_N, T, G, T, 4, 518)
        assert all(0 < r["nb"] <= 512 for r in four)
        assert any(r["blk_lo"] > 0 for r in four)
        tokens = V.long_tokens(T)
        for t in range(T):
            cand = tokens(0, t)
            assert min(cand) == 8191 and max(cand) == V.LONG_N - T + t
            assert {8191, 8192} <= set(cand)


# --------------------------------------------------------------------------
# the checkers on the reference, right and wrong
# --------------------------------------------------------------------------

def _ref(case, layout="plain"):
    """ops.paged_verify_ref in fp32 on the case."""
    kc, vc = V.host_caches(case, layout)
    return ops.paged_verify_ref(case.q.float(), kc.float(), vc.float(),
                                case.bt, case.seq_lens, case.q_lens,
                                case.scale)


def _real(case):
    """[B, T] bool: real query rows."""
    return torch.arange(case.T)[None, :] < case.q_lens[:, None]


def _wrong_table(case, want_far):
    """(b, table) pairs: sequence b's entry 0 pointing into a block of
    another sequence (its entry 1 where it has one and `want_far`, so that
    the block holds other census residues)."""
    for b in range(case.B):
        if case.need(b) == 0:
            continue
        other = [o for o in range(case.B) if o != b and
                 case.need(o) >= (2 if want_far else 1)]
        if not other:
            continue
        bt = case.bt.clone()
        bt[b, 0] = case.bt[other[0], 1 if want_far else 0]
        yield b, bt


def _wrong_keys(case, kref, vref):
    """(name, output, rows it must change [B, T]) of every one-wrong-key
    variant of the float64 reference."""
    real = _real(case)
    yield "limit + 1", V.ref64(case, kref, vref, shift=1), real
    yield "limit - 1", V.ref64(case, kref, vref, shift=-1), real
    yield "first key dropped", V.ref64(case, kref, vref, drop_first=True), \
        real


PARAMS = [pytest.param(dh, G, T, hkv, id=f"{dh}-G{G}-T{T}")
          for dh in V.DHS for G, T, hkv in V.SHAPES]
NPARAMS = [p for p in PARAMS if p.values[1] * p.values[2] <= p.values[0]]


@pytest.mark.parametrize("dh,G,T,hkv", PARAMS)
def test_census_cases(dh, G, T, hkv):
    for i, seqs in enumerate(V.length_batches(G, T)):
        case = V.census_case(dh, G, T, hkv, seqs, seed=10 * i + G + T)
        cnt, n = V.census_counts(case)
        assert float(cnt.max()) <= 128
        assert torch.equal(cnt.sum(dim=-1), n)
        # scattered table over the whole pool, ids inside it
        assert len(set(case.bt.flatten().tolist())) == case.k.shape[0]
        assert torch.isfinite(case.k.float()).all()
        for layout in V.LAYOUTS:
            assert V.census_error(_ref(case, layout), case) <= 0.25, layout
        assert V.census_error(V.ref64(case, case.k, case.v), case) <= 0.25
        real = _real(case)
        for name, out, rows in _wrong_keys(case, case.k, case.v):
            err = V.census_row_error(out, case)
            assert bool((err[rows] >= 0.5).all()), (name, seqs, err)
            assert bool((err[~real] == 0).all()), name
        for b, bt in _wrong_table(case, want_far=True):
            out = V.ref64(case, case.k, case.v, bt=bt)
            err = V.census_row_error(out, case)
            assert bool((err[b][real[b]] >= 0.5).all()), (seqs, b, err[b])
        # a padding row that is not zero fails
        out = V.ref64(case, case.k, case.v)
        if bool((~real).any()):
            out[~real] = 2.0 ** -20
            assert V.census_error(out, case) > 100


@pytest.mark.parametrize("dh,G,T,hkv", NPARAMS)
def test_needle_cases(dh, G, T, hkv):
    hit = set()
    for i, seqs in enumerate(V.length_batches(G, T)):
        for rnd in range(V.NEEDLE_ROUNDS):
            case = V.needle_case(dh, G, T, hkv, seqs, seed=10 * i + G + T,
                                 rnd=rnd)
            real = _real(case)
            assert bool((case.tau[~real] == -1).all())
            for b in range(case.B):
                ctx = case.ctx(b)
                for t in range(case.ql(b)):
                    tau = case.tau[b, t]
                    assert bool(((0 <= tau) & (tau <= ctx + t)).all())
                    for p in tau.tolist():
                        hit |= {("own", p == ctx + t), ("first", p == 0),
                                ("ctx", p - ctx), ("slot", p % BS)}
            for layout in V.LAYOUTS if rnd == 0 else ("plain",):
                err = V.needle_error(_ref(case, layout), case, case.v)
                assert err <= 1.0, (layout, seqs, rnd, err)
            # one key too many: the decoy, a dead slot or the poison block
            out = V.ref64(case, case.k, case.v, shift=1)
            err = V.needle_row_error(out, case, case.v)
            assert bool((err[real] > 100).all()), (seqs, rnd, err)
            # the needle's table entry pointing into another sequence
            for b in range(case.B):
                other = [o for o in range(case.B) if o != b and case.need(o)]
                if case.ql(b) == 0 or not other:
                    continue
                e = case.tau[b] // BS
                bt = case.bt.clone()
                bt[b, int(e[0, 0])] = case.bt[other[0], 0]
                out = V.ref64(case, case.k, case.v, bt=bt)
                err = V.ulp_error(out, V.needle_expected(case, case.v))
                moved = err[b].amax(dim=-1)[(e == e[0, 0]) & real[b][:, None]]
                assert bool((moved > 1.0).all()), (seqs, rnd, b)
    if T >= 2:
        assert {("ctx", -1), ("ctx", 0)} <= hit
    assert {("own", True), ("own", False), ("first", True),
            ("slot", 0), ("slot", 15)} <= hit


@pytest.mark.parametrize("dh,layout,G,T", V.LONG_SHAPES)
def test_long_case(dh, layout, G, T):
    """The 8245-key case: counts within the census bound, needles where the
    table is read from global memory, reference passes, one wrong key
    fails."""
    seqs = [(V.LONG_N, T)]
    case = V.census_case(dh, G, T, 1, seqs, seed=77, lo=V.long_census_lo(dh))
    cnt, n = V.census_counts(case)
    assert 2 <= float(cnt.max()) <= 128
    assert float(cnt[0, :, :].sum(-1).min()) >= dh + (V.LONG_N - T + 1 - 8191)
    assert V.census_error(_ref(case, layout), case) <= 0.25
    for name, out, rows in _wrong_keys(case, case.k, case.v):
        err = V.census_row_error(out, case)
        assert bool((err[rows] >= 0.5).all()), (name, err)
    for rnd in range(V.LONG_ROUNDS):
        case = V.needle_case(dh, G, T, 1, seqs, seed=78, rnd=rnd,
                             tokens=V.long_tokens(T))
        assert int(case.tau.min()) >= 8191
        assert V.needle_error(_ref(case, layout), case, case.v) <= 1.0
        out = V.ref64(case, case.k, case.v, shift=1)
        assert bool((V.needle_row_error(out, case, case.v) > 100).all())


def _random_cases():
    for dh in V.DHS:
        for G, T, hkv in V.SHAPES:
            if G * T <= dh:
                for case in V.random_cases(dh, G, T, hkv):
                    yield dh, G, T, case


def test_tau_table():
    """The measured column of the GPU module's table, and tau = 2 x it."""
    meas = 0.0
    for dh, G, T, case in _random_cases():
        ref = V.ref64(case, case.k, case.v)
        rnd = V.ref64(case, case.k, case.v, rounding=True)
        meas = max(meas, float(V.row_metric(rnd, ref).max()))
    print("measured", meas, "tau", V.TAU)
    assert 0.95 * V.TAU / 2 <= meas <= V.TAU / 2, meas
    assert V.TAU < 3e-2


@pytest.mark.parametrize("dh,G,T,hkv", NPARAMS)
def test_random_cases_are_sensitive(dh, G, T, hkv):
    """First and last visible key hold 5-30 % of every real row's mass; the
    fp32 reference is far inside tau; one wrong key moves every real row by
    at least 3 tau."""
    for case in V.random_cases(dh, G, T, hkv):
        real = _real(case)
        ref = V.ref64(case, case.k, case.v)
        assert torch.isfinite(case.k.float()).all()
        for layout in V.LAYOUTS:
            m = float(V.row_metric(_ref(case, layout), ref).max())
            assert m < V.TAU / 100, (layout, m)
        for b in range(case.B):
            ctx = case.ctx(b)
            kk = V.plain_rows(case.k, case, b).double()
            kk = kk.repeat_interleave(G, dim=1)
            for t in range(case.ql(b)):
                n = ctx + t + 1
                sc = torch.einsum("mhd,hd->mh", kk[:n + 1],
                                  case.q[b, t].double()) * case.scale
                p = torch.softmax(sc[:n], dim=0)
                for i in (0, -1):
                    assert 0.05 <= float(p[i].min()) and \
                        float(p[i].max()) <= 0.30, (b, t, i, p[i])
                # the key behind the limit would hold comparable mass
                extra = torch.softmax(sc, dim=0)[-1]
                assert float(extra.min()) >= 0.05, (b, t, extra)
        variants = list(_wrong_keys(case, case.k, case.v))
        for b, bt in _wrong_table(case, want_far=False):
            rows = torch.zeros_like(real)
            rows[b] = real[b]
            variants.append((f"table entry of {b}",
                             V.ref64(case, case.k, case.v, bt=bt), rows))
        for name, out, rows in variants:
            moved = V.row_metric(out, ref)[rows]
            assert float(moved.min()) >= 3 * V.TAU, \
                (name, float(moved.min()), V.TAU)


@pytest.mark.parametrize("dh,G,T,hkv", [PARAMS[3], PARAMS[-1]])
def test_invariant_cases(dh, G, T, hkv):
    """The bit-exact test's cases: padding rows are filled in q only, and
    the reference does not read them."""
    for i, seqs in enumerate(V.length_batches(G, T)):
        case = V.plain_random_case(dh, G, T, hkv, seqs, seed=300 + i + G + T)
        real = _real(case)
        qpad = V.pad_filled(case)
        assert bool((qpad[~real] == V.PAD_FILL).all())
        assert torch.equal(qpad[real], case.q[real])
        filled = dataclasses.replace(case, q=qpad)
        assert torch.equal(_ref(filled), _ref(case))
        assert not bool(_ref(case)[~real].any())
