"""int4 weight-only decode path (MODEL_LOAD_IN_4BIT), CPU side.

Covers the quantization format of ops/linear.py (quantize_int4 /
dequantize_int4 / fake_quantize_int4_), the registry rules, the env knob
and example manifests, and a CPU simulation of
ops/csrc/decode_gemm_w4.hip's index dataflow in the style of
test_gemm_sim_cpu.py: a Python mirror of w4_swizzle built from the
DOCUMENTED layout (not from the C++ expression), then a lane-by-lane walk
of the kernel's address arithmetic with the mfma_f32_32x32x16_bf16 A/B/C
lane maps, the per-wave group-range split, the LDS reduce and the slab
combine. What it cannot check is the intrinsic's true lane maps and the
hardware (covered on-GPU by tests/test_w4_gpu.py).

Keep in sync with decode_gemm_w4.hip when editing either.
"""
import weakref
from pathlib import Path

import numpy as np
import pytest
import torch

from runbooks_amd.ops import linear as L

ROOT = Path(__file__).resolve().parent.parent


# --------------------------------------------------------------------------
# weights that make a mis-indexed scale or nibble visible
# --------------------------------------------------------------------------
def spread_weights(n, k, seed, outliers=True):
    """randn with per-group magnitudes spread over [0.25, 4] (log-uniform)
    plus a few 20x outliers."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, k, generator=g)
    mag = 0.25 * 16.0 ** torch.rand(n, k // 64, generator=g)
    w = (w.reshape(n, k // 64, 64) * mag[:, :, None]).reshape(n, k)
    if outliers:
        idx = torch.randint(0, n * k, (max(4, n * k // 4096),), generator=g)
        w.view(-1)[idx] *= 20.0
    return w


def codes_of(q):
    """canonical q [N, K/2] -> int codes [N, K] in [-8, 7]."""
    q = q.to(torch.int32)
    return torch.stack([q & 0xF, q >> 4], dim=2).reshape(q.shape[0], -1) - 8


# --------------------------------------------------------------------------
# format
# --------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["randn", "spread"])
@pytest.mark.parametrize("n,k", [(256, 512), (5, 128), (96, 832)])
def test_roundtrip_bound(kind, n, k):
    """|w - dq| <= 0.51 * scale of the element's group (half a step plus
    the bf16 rounding of the scale); codes within [-7, 7]."""
    if kind == "randn":
        w = torch.randn(n, k, generator=torch.Generator().manual_seed(n + k))
    else:
        w = spread_weights(n, k, seed=n * k)
    q, s = L.quantize_int4(w)
    assert q.dtype == torch.uint8 and q.shape == (n, k // 2)
    assert s.dtype == torch.bfloat16 and s.shape == (n, k // 64)
    back = L.dequantize_int4(q, s, dtype=torch.float32)
    bound = 0.51 * s.float().repeat_interleave(64, dim=1)
    err = (w - back).abs()
    assert bool((err <= bound).all()), float((err / bound).max())
    c = codes_of(q)
    assert int(c.min()) >= -7 and int(c.max()) <= 7


def test_zero_group_is_exact_zero():
    w = torch.randn(4, 128, generator=torch.Generator().manual_seed(1))
    w[1, 64:] = 0.0
    w[3, :64] = -0.0
    q, s = L.quantize_int4(w)
    for dt in (torch.float32, torch.bfloat16):
        back = L.dequantize_int4(q, s, dtype=dt)
        assert bool((back[1, 64:] == 0).all())
        assert bool((back[3, :64] == 0).all())
    assert bool((q[1, 32:] == 0x88).all())      # code 0 -> nibble 8


def test_packing_nibble_order():
    """Hand-written 1x64 case: even k in the low nibble, odd k high."""
    w = torch.zeros(1, 64)
    w[0, 0] = 7.0        # absmax -> scale exactly 1.0
    w[0, 1] = -3.0
    w[0, 2] = 2.0
    w[0, 63] = -7.0
    q, s = L.quantize_int4(w)
    assert float(s[0, 0]) == 1.0
    assert int(q[0, 0]) == ((-3 + 8) << 4) | (7 + 8)      # k=1 high, k=0 low
    assert int(q[0, 1]) == ((0 + 8) << 4) | (2 + 8)       # k=3 high, k=2 low
    assert int(q[0, 31]) == ((-7 + 8) << 4) | (0 + 8)     # k=63 high
    back = L.dequantize_int4(q, s, dtype=torch.float32)
    assert torch.equal(back, w)


def test_fake_quantize_matches_dequantize_and_registers_nothing():
    L._W4_REGISTRY.clear()
    w = spread_weights(32, 256, seed=3).to(torch.bfloat16)
    q, s = L.quantize_int4(w)
    want = L.dequantize_int4(q, s, dtype=torch.bfloat16)
    got = L.fake_quantize_int4_(w.clone())
    assert torch.equal(got, want)
    assert len(L._W4_REGISTRY) == 0


def test_quantize_rejects_bad_k():
    with pytest.raises(ValueError):
        L.quantize_int4(torch.zeros(32, 96))


# --------------------------------------------------------------------------
# registry
# --------------------------------------------------------------------------
def test_cpu_quantize_registers_nothing():
    L._W4_REGISTRY.clear()
    w = torch.randn(32, 128)
    q, s = L.quantize_int4(w)
    assert not q.is_cuda and not s.is_cuda
    assert len(L._W4_REGISTRY) == 0
    assert L._registry_get(L._W4_REGISTRY, w) is None


def test_registry_weakref_identity():
    """A different tensor at a recycled data_ptr misses (and drops the
    stale entry); the registered tensor itself hits."""
    L._W4_REGISTRY.clear()
    a = torch.randn(32, 64)
    entry = (torch.zeros(1), torch.zeros(1), (32, 64), weakref.ref(a))
    L._W4_REGISTRY[a.data_ptr()] = entry
    assert L._registry_get(L._W4_REGISTRY, a) is entry
    b = a.data                       # same storage address, other object
    assert b is not a and b.data_ptr() == a.data_ptr()
    assert L._registry_get(L._W4_REGISTRY, b) is None
    assert a.data_ptr() not in L._W4_REGISTRY
    L._W4_REGISTRY.clear()


# --------------------------------------------------------------------------
# layout mirror + kernel dataflow simulation
# --------------------------------------------------------------------------
U = 4                # groups per ring half in the kernel


def w4_swizzle_mirror(q, scales):
    """Mirror of w4_swizzle, written from the documented layout:
    wq_swz [N/32][K/64][lane][16 B] where dword j of lane l holds, in bits
    4i..4i+3, the nibble of row l&31, k = kb*64 + j*16 + (l>>5)*8 + i;
    sc_swz [N/32][K/64][32]. Returns (uint8 [N/32,K/64,64,16] tensor,
    bf16 [N/32,K/64,32] tensor)."""
    n, kh = q.shape
    k = 2 * kh
    nib = (codes_of(q) + 8).numpy().astype(np.uint32)          # [N, K]
    nb, kb, lane, j, i = np.meshgrid(
        np.arange(n // 32), np.arange(k // 64), np.arange(64),
        np.arange(4), np.arange(8), indexing="ij")
    row = nb * 32 + (lane & 31)
    kk = kb * 64 + j * 16 + (lane >> 5) * 8 + i
    dwords = (nib[row, kk] << (4 * i).astype(np.uint32)).sum(
        axis=-1, dtype=np.uint64).astype("<u4")                # [..,64,4]
    wq = torch.from_numpy(
        np.ascontiguousarray(dwords).view(np.uint8).reshape(
            n // 32, k // 64, 64, 16).copy())
    sc = scales.view(torch.int16).numpy()
    nb, kb, r = np.meshgrid(np.arange(n // 32), np.arange(k // 64),
                            np.arange(32), indexing="ij")
    sc_swz = torch.from_numpy(sc[nb * 32 + r, kb].copy()).view(torch.bfloat16)
    return wq, sc_swz


def swizzle_x_mirror(x, M):
    """decode_swizzle_x: xs[s][lane][i] = x[lane&31][s*16 + (lane>>5)*8 + i],
    zero rows for m >= M. x float64 [M, K] -> [K/16, 64, 8]."""
    K = x.shape[1]
    xs = np.zeros((K // 16, 64, 8))
    for lane in range(64):
        m, hi = lane & 31, lane >> 5
        if m < M:
            for s in range(K // 16):
                xs[s, lane] = x[m, s * 16 + hi * 8:s * 16 + hi * 8 + 8]
    return xs


def w4_split_mirror(N, K):
    """Mirrors decode_gemm_w4_split."""
    nblocks, split = N // 32, 1
    while split < 8 and nblocks * split < 256 and \
            K // 64 >= 2 * U * 4 * (split * 2):
        split *= 2
    return split


def wave_range(groups_total, split, kslice, wid):
    """Mirrors the kernel's per-(kslice, wave) group range."""
    nranges = split * 4
    gpr = (groups_total + nranges - 1) // nranges
    g0 = min(groups_total, (kslice * 4 + wid) * gpr)
    g1 = min(groups_total, g0 + gpr)
    return g0, g1


def mfma_32x32x16(a_frags, b_frags, acc):
    """a_frags/b_frags [64 lanes, 8]; acc [64 lanes, 16 regs]. Documented
    maps: A lane l -> A[row l&31][k (l>>5)*8+i]; B lane l ->
    B[k (l>>5)*8+i][col l&31]; C lane l reg r ->
    C[row (r&3)+8*(r>>2)+4*(l>>5)][col l&31]."""
    A = np.zeros((32, 16))
    B = np.zeros((16, 32))
    for lane in range(64):
        r, hi = lane & 31, lane >> 5
        A[r, hi * 8:hi * 8 + 8] = a_frags[lane]
        B[hi * 8:hi * 8 + 8, r] = b_frags[lane]
    C = A @ B
    for lane in range(64):
        for reg in range(16):
            acc[lane, reg] += C[(reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5),
                                lane & 31]
    return acc


def simulate(xs, wq_swz, sc_swz, M, N, K, split):
    """Walk decode_gemm_w4_kernel (+ combine) and return y [M, N] f64."""
    wq = wq_swz.numpy().reshape(-1)                 # flat bytes
    sc = sc_swz.float().numpy().astype(np.float64).reshape(-1)
    xsf = xs.reshape(-1)
    groups_total = K // 64
    slabs = np.zeros((split, M, N))
    seen = np.zeros(groups_total * (N // 32), dtype=np.int64)
    for nblk in range(N // 32):
        wseg = nblk * groups_total * 1024
        sseg = nblk * groups_total * 32
        for kslice in range(split):
            red = np.zeros((4, 32, 32))
            for wid in range(4):
                g0, g1 = wave_range(groups_total, split, kslice, wid)
                acc = np.zeros((64, 16))
                # ring iterations and single-group tail visit g0..g1-1 in
                # order; the partition is checked in
                # test_ring_partition_covers_range
                for g in range(g0, g1):
                    seen[nblk * groups_total + g] += 1
                    a = np.zeros((4, 64, 8))
                    b = np.zeros((4, 64, 8))
                    for lane in range(64):
                        off = wseg + g * 1024 + lane * 16
                        raw = wq[off:off + 16].view("<u4")
                        s = sc[sseg + g * 32 + (lane & 31)]
                        for j in range(4):
                            w = int(raw[j])
                            even = w & 0x0F0F0F0F
                            odd = (w >> 4) & 0x0F0F0F0F
                            for byte in range(4):
                                ne = (even >> (8 * byte)) & 0xFF
                                no = (odd >> (8 * byte)) & 0xFF
                                a[j, lane, 2 * byte] = (ne - 8) * s
                                a[j, lane, 2 * byte + 1] = (no - 8) * s
                            xo = ((g * 4 + j) * 512) + lane * 8
                            b[j, lane] = xsf[xo:xo + 8]
                    for j in range(4):
                        mfma_32x32x16(a[j], b[j], acc)
                for lane in range(64):
                    for reg in range(16):
                        n_local = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
                        red[wid, n_local, lane & 31] = acc[lane, reg]
            for tid in range(256):
                em, en = tid >> 3, (tid & 7) * 4
                if em < M:
                    for j in range(4):
                        slabs[kslice, em, nblk * 32 + en + j] = \
                            red[:, en + j, em].sum()
    assert (seen == 1).all()            # every group read exactly once
    return slabs.sum(axis=0)


def test_ring_partition_covers_range():
    """Main ring (multiples of 2U) + single-group tail visit every group
    of a wave's range exactly once, for every range length in use."""
    for n in range(0, 40):
        g0 = 3
        g1 = g0 + n
        visited = []
        g = g0
        nmain = ((g1 - g0) // (2 * U)) * (2 * U)
        if nmain > 0:
            gmain = g0 + nmain
            while g + 2 * U <= gmain:
                visited += list(range(g, g + U))          # ring half A
                visited += list(range(g + U, g + 2 * U))  # ring half B
                g += 2 * U
        while g < g1:
            visited.append(g)
            g += 1
        assert visited == list(range(g0, g1)), n


def test_wave_ranges_uneven_and_empty():
    # 13 groups over 4 waves: 4,4,4,1; over 8 ranges: 2 x6, 1, empty
    assert [wave_range(13, 1, 0, w) for w in range(4)] == \
        [(0, 4), (4, 8), (8, 12), (12, 13)]
    r = [wave_range(13, 2, ks, w) for ks in range(2) for w in range(4)]
    assert r[:7] == [(0, 2), (2, 4), (4, 6), (6, 8), (8, 10), (10, 12),
                     (12, 13)]
    assert r[7] == (13, 13)
    # one group: three idle waves
    assert [wave_range(1, 1, 0, w) for w in range(4)] == \
        [(0, 1), (1, 1), (1, 1), (1, 1)]
    assert w4_split_mirror(4096, 4096) == 2
    assert w4_split_mirror(4096, 11008) == 2
    assert w4_split_mirror(12288, 4096) == 1
    assert w4_split_mirror(96, 832) == 1


def test_swizzle_mirror_is_a_byte_permutation():
    """The layout comment's claim: dword j of lane l is canonical bytes
    [row][(kb*64 + j*16 + (l>>5)*8)/2 .. +3]."""
    q, s = L.quantize_int4(spread_weights(64, 256, seed=5))
    wq, sc = w4_swizzle_mirror(q, s)
    for nb, kb, lane, j in [(0, 0, 0, 0), (1, 3, 37, 2), (0, 2, 63, 3),
                            (1, 1, 31, 1)]:
        c0 = (kb * 64 + j * 16 + (lane >> 5) * 8) // 2
        assert torch.equal(wq[nb, kb, lane, j * 4:j * 4 + 4],
                           q[nb * 32 + (lane & 31), c0:c0 + 4])
        assert sc[nb, kb, lane & 31] == s[nb * 32 + (lane & 31), kb]


@pytest.mark.parametrize("M,N,K,split", [
    (5, 64, 256, 1),
    (32, 96, 832, 1),      # 13 groups: uneven wave split 4,4,4,1
    (32, 96, 832, 2),      # slabs + combine, one EMPTY wave range
])
def test_kernel_dataflow_matches_matmul(M, N, K, split):
    w = spread_weights(N, K, seed=N + K)
    q, s = L.quantize_int4(w)
    g = torch.Generator().manual_seed(M)
    x = torch.randn(M, K, generator=g, dtype=torch.float64).numpy()
    wq_swz, sc_swz = w4_swizzle_mirror(q, s)
    y = simulate(swizzle_x_mirror(x, M), wq_swz, sc_swz, M, N, K, split)
    ref = x @ L.dequantize_int4(q, s, dtype=torch.float64).numpy().T
    assert y.shape == (M, N)
    assert np.allclose(y, ref, rtol=0, atol=1e-9 * np.abs(ref).max()), \
        np.abs(y - ref).max()


# --------------------------------------------------------------------------
# env knob + manifests
# --------------------------------------------------------------------------
@pytest.mark.parametrize("value,want", [("true", True), ("1", True),
                                        (None, False)])
def test_server_main_passes_load_in_4bit(tmp_path, monkeypatch, value, want):
    """server_main reads MODEL_LOAD_IN_4BIT and hands it to Engine
    (isolated like test_server_main_builds_engine: serve_forever patched
    out, Engine wrapped to record its keyword arguments)."""
    import json

    import runbooks_amd.serve as serve_mod
    import runbooks_amd.serve.http as http_mod
    from runbooks_amd.workloads import server_main
    model_dir = tmp_path / "model"
    model_dir.mkdir()
    (model_dir / "config.json").write_text(
        json.dumps({"runbooks_amd_config": "tiny-llama"}))
    monkeypatch.setenv("MODEL_DIR", str(model_dir))
    monkeypatch.delenv("TP", raising=False)
    monkeypatch.delenv("MODEL_LOAD_IN_8BIT", raising=False)
    if value is None:
        monkeypatch.delenv("MODEL_LOAD_IN_4BIT", raising=False)
    else:
        monkeypatch.setenv("MODEL_LOAD_IN_4BIT", value)

    seen = {}
    real_engine = serve_mod.Engine

    def recording_engine(model, **kw):
        seen.update(kw)
        return real_engine(model, **kw)

    monkeypatch.setattr(serve_mod, "Engine", recording_engine)
    monkeypatch.setattr(http_mod, "serve_forever",
                        lambda engine, tok, port, model_name: None)
    try:
        assert server_main.main() == 0
    finally:
        L._W4_REGISTRY.clear()
    assert seen["load_in_4bit"] is want
    assert seen["load_in_8bit"] is False


@pytest.mark.parametrize("path,model", [
    ("examples/llama2-70b/server-4bit.yaml", "llama-2-70b"),
    ("examples/falcon-40b/server-4bit.yaml", "falcon-40b"),
])
def test_4bit_example_manifests_roundtrip(path, model):
    import yaml

    from runbooks_amd.api import Server
    from runbooks_amd.api.types import object_from_manifest
    d = yaml.safe_load((ROOT / path).read_text())
    obj = object_from_manifest(d)
    assert isinstance(obj, Server)
    assert obj.env["MODEL_LOAD_IN_4BIT"] == "true"
    assert obj.resources.gpu.count == 1
    assert obj.resources.gpu.type == "amd-mi355x"
    back = obj.to_dict()
    assert back["spec"]["env"] == d["spec"]["env"]
    assert back["spec"]["model"]["name"] == model
    assert back["spec"]["resources"]["gpu"]["count"] == 1


def test_reference_4bit_manifests_set_the_knob():
    """The reference's two largest serving examples set exactly the knob
    server_main now reads."""
    import yaml
    for name in ("llama2-70b", "falcon-40b"):
        d = yaml.safe_load((ROOT / "tests/golden/reference_examples" / name /
                            "server.yaml").read_text())
        assert d["spec"]["env"]["MODEL_LOAD_IN_4BIT"].lower() in ("1", "true")
