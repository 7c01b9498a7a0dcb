"""CPU mirror of the row-permuted decode weight layouts and the fused
decode-GEMM epilogues' index maps (ops/csrc/decode_gemm.hip).

The decode GEMM's swizzled weight copy may hold its rows permuted
(glu16: 16 gate rows + the matching 16 up rows per 32-row block; rope16:
16 rows d + their rotate-half partners d + Dh/2 per q/k block) so that a
workgroup's epilogue holds both halves of every pair. This file mirrors,
in numpy, decode_swizzle_w_layout's permutations, epi_col (the
un-permuting store) and the fused epilogues' address arithmetic — the
down-proj operand offset, q_out, and the paged-cache offsets for the plain
and transposed-V layouts — and checks them against straightforward
references. It validates the index logic; the GPU tests check the kernel.

Keep in sync with decode_gemm.hip when editing either.
"""
import numpy as np
import pytest

BS = 16                      # cache block size (ops.BLOCK_SIZE)


# ---- decode_swizzle_w_layout ------------------------------------------------
def glu16_perm(inter):
    """perm[r] = original row held at permuted row r of the [2I, K] weight."""
    n = 2 * inter
    r = np.arange(n)
    b, l = r // 32, r % 32
    return np.where(l < 16, 0, n // 2 - 16) + 16 * b + l


def rope16_perm(hq, hkv, dh):
    n = (hq + 2 * hkv) * dh
    r = np.arange(n)
    b, l = r // 32, r % 32
    bph = dh // 32
    head, j = b // bph, b % bph
    qk = head * dh + 16 * j + (l & 15) + np.where(l < 16, 0, dh // 2)
    return np.where(head >= hq + hkv, r, qk)


# ---- epi_col: original column of local row en of block nblk -----------------
def col_glu(nblk, en, inter):
    return (0 if en < 16 else inter - 16) + nblk * 16 + en


def col_rope(nblk, en, hq, hkv, dh):
    bph = dh // 32
    head = nblk // bph
    if head >= hq + hkv:
        return nblk * 32 + en
    j = nblk - head * bph
    return head * dh + 16 * j + (en & 15) + (0 if en < 16 else dh // 2)


GLU_I = [16, 1040, 11008]
ROPE_SHAPES = [(hq, hkv, dh) for dh in (64, 128, 256)
               for hq, hkv in ((8, 8), (8, 2), (16, 1))]


@pytest.mark.parametrize("inter", GLU_I)
def test_glu16_perm_is_bijection_and_store_inverts_it(inter):
    perm = glu16_perm(inter)
    assert np.array_equal(np.sort(perm), np.arange(2 * inter))
    for nblk in range(inter // 16):
        for en in range(0, 32, 4):
            c = col_glu(nblk, en, inter)
            assert c % 4 == 0        # the 8-byte bf16 store stays aligned
            assert np.array_equal(perm[nblk * 32 + en:nblk * 32 + en + 4],
                                  c + np.arange(4))
        # local rows 0..15 = gate, 16..31 = the SAME columns of up
        rows = perm[nblk * 32:nblk * 32 + 32]
        assert np.array_equal(rows[:16], 16 * nblk + np.arange(16))
        assert np.array_equal(rows[16:], rows[:16] + inter)


@pytest.mark.parametrize("hq,hkv,dh", ROPE_SHAPES)
def test_rope16_perm_is_bijection_and_store_inverts_it(hq, hkv, dh):
    perm = rope16_perm(hq, hkv, dh)
    n = (hq + 2 * hkv) * dh
    assert np.array_equal(np.sort(perm), np.arange(n))
    bph = dh // 32
    for nblk in range(n // 32):
        for en in range(0, 32, 4):
            c = col_rope(nblk, en, hq, hkv, dh)
            assert c % 4 == 0
            assert np.array_equal(perm[nblk * 32 + en:nblk * 32 + en + 4],
                                  c + np.arange(4))
        rows = perm[nblk * 32:nblk * 32 + 32]
        head = nblk // bph
        # a block never straddles heads
        assert np.all(rows // dh == head)
        if head < hq + hkv:          # q/k: (d, d + Dh/2) pairs
            assert np.all(rows[:16] % dh < dh // 2)
            assert np.array_equal(rows[16:], rows[:16] + dh // 2)
        else:                        # v: identity
            assert np.array_equal(rows, nblk * 32 + np.arange(32))


# ---- fused GLU epilogue ----------------------------------------------------
def swizzle_x(h):
    """decode_swizzle_x: [M, K] -> [K/16][lane = hi*32 + m][8]; rows
    m >= M left as NaN here (unwritten on the GPU)."""
    m_rows, k = h.shape
    out = np.full((k // 16, 64, 8), np.nan)
    for s in range(k // 16):
        for hi in range(2):
            out[s, hi * 32:hi * 32 + m_rows] = \
                h[:, s * 16 + hi * 8:s * 16 + hi * 8 + 8]
    return out.reshape(-1)


def glu_epilogue(y_perm, m_rows, inter):
    """Mirror of the EPI_SWIGLU epilogue: y_perm [M, 2I] is the plain
    matmul against the PERMUTED weight (column = permuted row)."""
    swz = np.full((inter // 16) * 512, np.nan)
    for nblk in range(inter // 16):
        red = y_perm[:, nblk * 32:nblk * 32 + 32].T      # [local row][m]
        for tid in range(64):
            m = tid & 31
            if m >= m_rows:
                continue
            r0 = (tid >> 5) * 8
            for i in range(8):
                g, u = red[r0 + i, m], red[16 + r0 + i, m]
                swz[nblk * 512 + tid * 8 + i] = g / (1.0 + np.exp(-g)) * u
    return swz


@pytest.mark.parametrize("m_rows,inter", [(1, 16), (5, 1040), (32, 48)])
def test_glu_epilogue_reproduces_swiglu_in_operand_order(m_rows, inter):
    rng = np.random.default_rng(inter + m_rows)
    k = 64
    x = rng.standard_normal((m_rows, k))
    w = rng.standard_normal((2 * inter, k))
    y_perm = x @ w[glu16_perm(inter)].T
    g, u = x @ w[:inter].T, x @ w[inter:].T
    want = swizzle_x(g / (1.0 + np.exp(-g)) * u)
    got = glu_epilogue(y_perm, m_rows, inter)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0, equal_nan=True)


# ---- fused RoPE + append epilogue ------------------------------------------
def rope_epilogue(y_perm, pos, slots, cos, sin, hq, hkv, dh, nblocks, vt):
    """Mirror of EPI_ROPE / EPI_ROPE_VT over every workgroup and thread;
    returns flat q_out, k_cache, v_cache (NaN = never written)."""
    m_rows = y_perm.shape[0]
    half = dh // 2
    q = np.full(m_rows * hq * dh, np.nan)
    kc = np.full(nblocks * hkv * BS * dh, np.nan)
    vc = np.full(nblocks * hkv * BS * dh, np.nan)
    bph = dh // 32
    for nblk in range(y_perm.shape[1] // 32):
        red = y_perm[:, nblk * 32:nblk * 32 + 32].T
        head = nblk // bph
        j = nblk - head * bph
        for tid in range(256):
            em, sub = tid >> 3, tid & 7
            if em >= m_rows:
                continue
            slot = slots[em]
            if head < hq + hkv:
                p = sub * 2
                d = 16 * j + p
                if head < hq:
                    dst, buf = (em * hq + head) * dh + d, q
                else:
                    if slot < 0:
                        continue
                    dst = (((slot // BS) * hkv + (head - hq)) * BS +
                           slot % BS) * dh + d
                    buf = kc
                toff = pos[em] * half + d
                for e in range(2):
                    a, b = red[p + e, em], red[16 + p + e, em]
                    c, s = cos.reshape(-1)[toff + e], sin.reshape(-1)[toff + e]
                    buf[dst + e] = a * c - b * s
                    buf[dst + half + e] = b * c + a * s
            else:
                if slot < 0:
                    continue
                hv = head - hq - hkv
                en = sub * 4
                d = 32 * j + en
                for i in range(4):
                    if vt:
                        vbase = ((slot // BS) * hkv + hv) * dh * BS
                        vc[vbase + (d + i) * BS + slot % BS] = red[en + i, em]
                    else:
                        vc[(((slot // BS) * hkv + hv) * BS + slot % BS) * dh
                           + d + i] = red[en + i, em]
    return q, kc, vc


@pytest.mark.parametrize("vt", [False, True])
@pytest.mark.parametrize("hq,hkv,dh", [(2, 2, 64), (4, 1, 128), (2, 2, 256)])
def test_rope_epilogue_reproduces_rotate_half_and_cache_append(hq, hkv, dh,
                                                               vt):
    rng = np.random.default_rng(hq * 100 + dh)
    m_rows, k, nblocks, half = 5, 32, 3, dh // 2
    n = (hq + 2 * hkv) * dh
    x = rng.standard_normal((m_rows, k))
    w = rng.standard_normal((n, k))
    pos = np.array([7, 2, 9, 0, 4])                  # non-monotonic
    slots = np.array([3, 17, -1, 40, 18])            # three blocks, one skip
    ang = rng.standard_normal((10, half))
    cos, sin = np.cos(ang), np.sin(ang)

    y_perm = x @ w[rope16_perm(hq, hkv, dh)].T
    q, kc, vc = rope_epilogue(y_perm, pos, slots, cos, sin, hq, hkv, dh,
                              nblocks, vt)

    # straightforward reference on the unpermuted product
    y = (x @ w.T).reshape(m_rows, hq + 2 * hkv, dh)

    def rot(t):                                      # [M, H, Dh]
        a, b = t[..., :half], t[..., half:]
        c, s = cos[pos][:, None, :], sin[pos][:, None, :]
        return np.concatenate([a * c - b * s, b * c + a * s], axis=-1)

    q_ref = rot(y[:, :hq])
    k_ref = rot(y[:, hq:hq + hkv])
    v_ref = y[:, hq + hkv:]
    kc_ref = np.full((nblocks, hkv, BS, dh), np.nan)
    vc_ref = np.full((nblocks, hkv, dh, BS) if vt else (nblocks, hkv, BS, dh),
                     np.nan)
    for m, slot in enumerate(slots):
        if slot < 0:
            continue
        kc_ref[slot // BS, :, slot % BS] = k_ref[m]
        if vt:
            vc_ref[slot // BS, :, :, slot % BS] = v_ref[m]
        else:
            vc_ref[slot // BS, :, slot % BS] = v_ref[m]
    for got, want in ((q, q_ref), (kc, kc_ref), (vc, vc_ref)):
        want = want.reshape(-1)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0,
                                   equal_nan=True)
