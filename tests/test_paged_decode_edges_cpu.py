"""CPU proof that tests/test_paged_decode_edges_gpu.py would notice a
subtly wrong decode kernel, without ever running one.

For every case its builders make, the fp32 reference (ops.paged_decode_ref)
and the numpy model of the kernel's split / window index math
(simulate_decode) pass the very checkers the GPU tests use, and the same
reference fed ONE wrong key -- the poison key after the last live one, the
poison key before the window, one live key lost, a table entry that
points into another sequence's block -- fails them. The random test's tolerance table is recomputed
here, and its cases are shown to move by at least three tolerances when
the first or last live key is lost or a poison key is added.
"""
import pytest
import torch

from runbooks_amd import ops

import test_paged_decode_edges_gpu as E
from test_decode_sim_cpu import simulate_decode

WINDOWED = [False, True]


def _ref(case, kc, vc, lens=None, starts=None):
    """ops.paged_decode_ref in fp32 on the case (or on changed bounds)."""
    st = case.starts if starts is None else starts
    return ops.paged_decode_ref(
        case.q.float(), kc if kc.dtype == torch.uint8 else kc.float(),
        vc if vc.dtype == torch.uint8 else vc.float(), case.bt,
        case.lens if lens is None else lens, case.scale, seq_starts=st)


def _sim(case, nsplit):
    out = simulate_decode(
        case.q.double().numpy(), case.k.double().numpy(),
        case.v.double().numpy(), case.bt.numpy(), case.lens.numpy(),
        case.scale, nsplit=nsplit,
        seq_starts=None if case.starts is None else case.starts.numpy())
    return torch.from_numpy(out)


def _batches(windowed):
    for i, lengths in enumerate(E.LENGTH_BATCHES):
        if windowed:
            yield i, E.with_starts(lengths, rot=i)
        else:
            yield i, (lengths, None)


def _wrong_bounds(case):
    """(name, lens, starts, rows it changes) for one extra or lost key."""
    one = torch.ones_like(case.lens)
    live = case.lens - (case.starts if case.starts is not None else 0)
    every = torch.ones_like(one, dtype=torch.bool)
    yield "poison key at seq_len", case.lens + one, case.starts, every
    yield "last key lost", case.lens - one, case.starts, live >= 1
    if case.starts is not None:
        yield "poison key before the window", case.lens, \
            case.starts - one, case.starts >= 1
        yield "first key lost", case.lens, case.starts + one, live >= 1


def test_lengths_reach_every_trip_count():
    """The length list walks trip counts 1..5 (both edges) at every stride
    of the scalar kernel, the MFMA block counts 1, 4, 5, 8, 9 and the
    issue's fixed lengths."""
    lengths = {n for row in E.LENGTH_BATCHES for n in row}
    assert {1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 0, 5} <= lengths
    for stride in (4, 8, 16, 32):
        trips = {(n + stride - 1) // stride for n in lengths}
        assert {1, 2, 3, 4, 5} <= trips, stride
        for trip in (1, 2, 3, 4):       # last full step and one past it
            assert {trip * stride, trip * stride + 1} <= lengths, \
                (stride, trip)
    for depth in (2, 4):                # ring tail: every niter mod DEPTH
        assert {((n + 3) // 4) % depth for n in lengths if n} == \
            set(range(depth))
    assert {1, 4, 5, 8, 9} <= {(n + 15) // 16 for n in lengths}


@pytest.mark.parametrize("windowed", WINDOWED)
@pytest.mark.parametrize("dh,G", E.INSTANCES)
def test_census_cases(dh, G, windowed):
    for i, (lens, starts) in _batches(windowed):
        case = E.census_case(dh, G, lens, starts, seed=10 * i + G)
        cnt = E.census_counts(case)
        assert float(cnt.max()) <= 64          # <= 128, and fp8 MFMA's 64
        assert int(cnt.sum()) == sum(lens) - sum(starts or [0])
        # scattered table: live entries are not an arange
        assert len(set(case.bt.flatten().tolist())) == case.k.shape[0]
        for layout in E.layouts_for(G):
            kc, vc, _, _, _ = E.host_caches(case, layout)
            assert E.census_error(_ref(case, kc, vc), case) <= 0.25, layout
        ns = E.NSPLITS[(i + G) % 4] if 5 not in lens else 16
        assert E.census_error(_sim(case, ns), case) <= 0.25, ns
        # one wrong key, in every row it can be wrong in
        for name, wl, ws, rows in _wrong_bounds(case):
            out = _ref(case, case.k, case.v, lens=wl, starts=ws)
            for b in torch.nonzero(rows).flatten().tolist():
                err = E.census_error(out[b:b + 1], E._row_case(case, b))
                assert err >= 0.75, (name, lens, starts, b, err)


@pytest.mark.parametrize("windowed", WINDOWED)
@pytest.mark.parametrize("dh,G", E.INSTANCES)
def test_needle_cases(dh, G, windowed):
    hit = set()
    for i, (lens, starts) in _batches(windowed):
        for rnd in range(E.NEEDLE_ROUNDS["plain"]):
            case = E.needle_case(dh, G, lens, starts, seed=10 * i + G,
                                 rnd=rnd)
            for b in range(case.B):
                n, s = int(case.lens[b]), case.start(b)
                for t in case.tau[b]:
                    assert (s <= t < n) if n > s else t == -1
                    hit |= {("first", t == s), ("last", t == n - 1),
                            ("slot", t % 16)}
            lays = E.layouts_for(G) if rnd < 1 else ("plain",)
            for layout in lays:
                kc, vc, _, vref, _ = E.host_caches(case, layout)
                err = E.needle_error(_ref(case, kc, vc), case, vref)
                assert err <= 1.0, (layout, err)
            if rnd == 0:
                ns = E.NSPLITS[(i + G) % 4] if 5 not in lens else 16
                assert E.needle_error(_sim(case, ns), case, case.v) <= 1.0
            # an attended poison key takes the mass from every needle
            for name, wl, ws, rows in _wrong_bounds(case):
                if "poison" not in name:
                    continue
                out = _ref(case, case.k, case.v, lens=wl, starts=ws)
                for b in torch.nonzero(rows).flatten().tolist():
                    err = E.needle_error(out[b:b + 1], E._row_case(case, b),
                                         case.v)
                    assert err > 100, (name, lens, starts, b, err)
            # the permuted table makes a wrong block visible: read the
            # needle's entry from another sequence's block
            for b in range(case.B):
                other = [x for x in range(case.B) if x != b and
                         int(case.lens[x]) > case.start(x)]
                if case.tau[b][0] < 0 or not other:
                    continue
                o = other[0]
                wrong = E._row_case(case, b)
                wrong = E.dataclasses.replace(wrong, bt=wrong.bt.clone())
                wrong.bt[0, case.tau[b][0] // 16] = \
                    case.bt[o, case.start(o) // 16]
                out = _ref(wrong, case.k, case.v)
                right = E._row_case(case, b)
                assert E.needle_error(out, right, case.v) > 1.0, (lens, b)
    assert {("first", True), ("last", True)} <= hit
    assert {("slot", 0), ("slot", 15)} <= hit


@pytest.mark.parametrize("G", [1, 4])
def test_long_case(G):
    """The > 8192-key case: counts within the census bound, needles where
    the table is read from global memory, reference and index model pass."""
    case = E.census_case(128, G, [E.LONG_N], None, seed=77, hkv=1)
    assert E.LONG_N > 8192 and (E.LONG_N + 15) // 16 > 512
    assert 64 < float(E.census_counts(case).max()) <= 128
    assert E.census_error(_ref(case, case.k, case.v), case) <= 0.25
    assert E.census_error(_sim(case, 4 if G == 4 else 1), case) <= 0.25
    out = _ref(case, case.k, case.v, lens=case.lens + 1)
    assert E.census_error(out, case) >= 0.75
    for rnd in range(len(E.LONG_NEEDLES) // G):
        case = E.needle_case(128, G, [E.LONG_N], None, seed=78, rnd=rnd,
                             tokens=[E.LONG_NEEDLES], hkv=1)
        assert sorted(case.tau[0]) == sorted(
            E.LONG_NEEDLES[rnd * G:(rnd + 1) * G])
        assert E.needle_error(_ref(case, case.k, case.v), case,
                              case.v) <= 1.0
        out = _ref(case, case.k, case.v, lens=case.lens + 1)
        assert E.needle_error(out, case, case.v) > 100


def _random_layout_cases():
    for dh, G in E.INSTANCES:
        for case in E.random_cases(dh, G):
            for layout in E.layouts_for(G):
                yield dh, G, layout, case


def test_tau_table():
    """The measured column of the GPU module's table, and tau = 2 x it."""
    meas = dict.fromkeys(E.TAU, 0.0)
    for dh, G, layout, case in _random_layout_cases():
        _, _, kref, vref, vs = E.host_caches(case, layout)
        cls = E.path_class(G, layout)
        ref = E.ref64(case, kref, vref)
        rnd = E.ref64(case, kref, vref, rounding=cls, vscale=vs)
        meas[cls] = max(meas[cls], float(E.row_metric(rnd, ref).max()))
    print("measured", meas)
    for cls, m in meas.items():
        # the table rounds the measurement up to three digits
        assert 0.95 * E.TAU[cls] / 2 <= m <= E.TAU[cls] / 2, (cls, m)


@pytest.mark.parametrize("dh,G", E.INSTANCES)
def test_random_cases_are_sensitive(dh, G):
    """First and last live key hold 5-30 % of every row's mass, and one
    lost or extra key moves every row of its sequence by >= 3 tau; the
    fp32 reference itself is far inside tau."""
    for case in E.random_cases(dh, G):
        assert case.B * case.q.shape[1] <= 64
        for layout in E.layouts_for(G):
            kc, vc, kref, vref, _ = E.host_caches(case, layout)
            tau = E.TAU[E.path_class(G, layout)]
            ref = E.ref64(case, kref, vref)
            assert float(E.row_metric(_ref(case, kc, vc), ref).max()) < \
                tau / 100
            for b in range(case.B):
                n, s = int(case.lens[b]), case.start(b)
                kk = E.plain_rows(kref, case, b)[s:n].double()
                kk = kk.repeat_interleave(G, dim=1)
                sc = torch.einsum("mhd,hd->mh", kk,
                                  case.q[b].double()) * case.scale
                p = torch.softmax(sc, dim=0)
                for i in (0, -1):
                    assert 0.05 <= float(p[i].min()) and \
                        float(p[i].max()) <= 0.30, (layout, b, i, p[i])
            changed = [
                ("first key lost", E.ref64(case, kref, vref, drop=0)),
                ("last key lost", E.ref64(case, kref, vref, drop=-1)),
                ("poison key at seq_len",
                 E.ref64(case, kref, vref, lens=case.lens + 1)),
            ]
            if case.starts is not None:
                changed.append(("poison key before the window", E.ref64(
                    case, kref, vref, starts=case.starts - 1)))
            for name, out in changed:
                moved = float(E.row_metric(out, ref).min())
                assert moved >= 3 * tau, (layout, name, moved, tau)


def test_old_tolerance_was_blind():
    """What the issue measured: at allclose(3e-2, 3e-2) a lost last key
    of a 170-key randn sequence mostly passes; this module's random case
    of the same size notices at every row."""
    torch.manual_seed(0)
    miss = 0
    for seed in range(8):
        g = torch.Generator().manual_seed(seed)
        q = torch.randn(1, 8, 128, generator=g).bfloat16().float()
        k = torch.randn(11, 8, 16, 128, generator=g).bfloat16().float()
        v = torch.randn(11, 8, 16, 128, generator=g).bfloat16().float()
        bt = torch.arange(11, dtype=torch.int32)[None]
        a = ops.paged_decode_ref(q, k, v, bt, torch.tensor([170]), 128 ** -.5)
        b = ops.paged_decode_ref(q, k, v, bt, torch.tensor([169]), 128 ** -.5)
        miss += bool(torch.allclose(a, b, atol=3e-2, rtol=3e-2))
    assert miss >= 1
    assert max(E.TAU.values()) < 3e-2
