"""Sliding-window prefill on the GPU (the WIN instantiations of
flash_fwd_core.h) at the edges of its geometry: 64-key tiles, 32-key
sub-tiles, 32-row waves, 256-row workgroups."""
import dataclasses

import pytest
import torch

from runbooks_amd import ops
from runbooks_amd.models import build_model, get_config
from test_window_prefill_cpu import attn64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BS = ops.BLOCK_SIZE
WINDOWS = (1, 31, 32, 33, 64, 65, 100, 257, 300, None)      # None: S + 7
SHAPES = ((4, 4, 64), (8, 2, 128))
# every window with both shapes at S = 530 and with one of them at 70 and
# 300; head_dim 256 with the window's edge inside a sub-tile
CASES = [(S, W or S + 7, shape) for S in (70, 300, 530)
         for i, W in enumerate(WINDOWS)
         for shape in (SHAPES if S == 530 else SHAPES[i % 2:][:1])]
CASES += [(530, 33, (2, 1, 256)), (530, 300, (2, 1, 256))]


@pytest.mark.parametrize("S,W,shape", CASES)
def test_census(S, W, shape):
    """q = 0 and V one-hot in j % Dh: out[p, d] * n_p counts the keys of
    (p - W, p] congruent to d. A lost, extra or shifted key moves a count
    by 1, bf16 rounding of out by at most count * 2^-9 < 0.02."""
    Hq, Hkv, D = shape
    q = torch.zeros(1, S, Hq, D, dtype=torch.bfloat16, device=DEV)
    k = torch.randn(1, S, Hkv, D, dtype=torch.bfloat16, device=DEV)
    hot = (torch.arange(S)[:, None] % D == torch.arange(D)[None]).float()
    v = hot.to(DEV, torch.bfloat16)[None, :, None].expand(1, S, Hkv, D)
    out = ops.flash_prefill(q, k, v.contiguous(), window=W)[0].float().cpu()
    d = torch.arange(S)[:, None] - torch.arange(S)[None]            # p - j
    count = ((d >= 0) & (d < W)).float() @ hot                      # [S, D]
    n = (torch.arange(S) + 1).clamp(max=W)
    err = (out * n[:, None, None] - count[:, None]).abs().max().item()
    print(f"census S={S} W={W} {shape}: max |out * n - count| = {err:.4f}")
    assert err <= 0.25


@pytest.mark.parametrize("S,W,shape", CASES)
def test_randn_against_float64(S, W, shape):
    """Per kv head one decoy on the key just outside a row's window:
    k[p0 - W] = 8 * q[p0], v = 100 there. q[..., 0] is +8 in the decoy's row
    and -8 in every other, so the rows that do see that key give it no
    weight (at weight P, v = 100 costs 100 * P * 2^-9 of bf16 rounding)."""
    Hq, Hkv, D = shape
    g = Hq // Hkv
    torch.manual_seed(S * 1000 + W)
    q, k, v = (torch.randn(S, h, D).bfloat16() for h in (Hq, Hkv, Hkv))
    q[:, :, 0] = -8
    rows = [p for p in (W, (W + S) // 2, S - 1) if W <= p < S][:Hkv]
    for h, p0 in enumerate(rows):
        q[p0, h * g:(h + 1) * g, 0] = 8
        k[p0 - W, h], v[p0 - W, h] = 8 * q[p0, h * g], 100
    qd, kd, vd = (t[None].to(DEV) for t in (q, k, v))
    out = ops.flash_prefill(qd, kd, vd, window=W)
    diff = (out[0].cpu().double() - attn64(q, k, v, W)).abs().max().item()
    print(f"randn S={S} W={W} {shape}: max abs diff vs float64 {diff:.3e}")
    assert diff < 3e-2
    if W >= S:      # a window over every key is no window, bit for bit
        assert torch.equal(out, ops.flash_prefill(qd, kd, vd))


@pytest.mark.parametrize("vt", [False, True])
@pytest.mark.parametrize("W", [33, 100, 300])
@pytest.mark.parametrize("ctx", [0, 48, 272])
def test_paged_window_matches_dense(ctx, W, vt):
    """paged_prefill(window) == rows [ctx:] of flash_prefill(window), with
    the table entries in front of the first workgroup's first tile and the
    trailing ones on an all-NaN spare block; batch rows == each alone."""
    Hq, Hkv, D = SHAPES[vt]
    T, T2, S = 300, 70, ctx + 300
    torch.manual_seed(ctx + W)
    q, k, v = (torch.randn(S, h, D, dtype=torch.bfloat16, device=DEV)
               for h in (Hq, Hkv, Hkv))
    nb = (S + BS - 1) // BS
    perm = torch.randperm(nb + 2)
    spare = perm[nb:nb + 1]
    full = torch.cat([perm[:nb], spare.repeat(3)]).to(torch.int32)
    kc, vc = ops.alloc_kv_cache(nb + 2, Hkv, D, DEV, v_transposed=vt)
    pos = torch.arange(S)
    ops.kv_append(k, v, kc, vc,
                  (full[pos // BS].long() * BS + pos % BS).int().to(DEV))
    kc[spare] = vc[spare] = float("nan")
    lazy = full.clone()
    lazy[:4 * (max(0, ctx - W + 1) // 64)] = spare
    full, lazy = full.to(DEV), lazy.to(DEV)
    out = ops.paged_prefill(q[ctx:], kc, vc, lazy, ctx, window=W)
    assert not torch.isnan(out.float()).any(), "an unneeded block was read"
    dense = ops.flash_prefill(q[None], k[None], v[None], window=W)[0]
    assert torch.equal(out, dense[ctx:])
    # the same chunk batched with a 70-token sequence on the same blocks
    plan = ops.paged_prefill_plan([T, T2], [ctx, 0], DEV)
    outb = ops.paged_prefill_batch(torch.cat([q[ctx:], q[:T2]]), kc, vc,
                                   torch.stack([lazy, full]), plan, window=W)
    assert torch.equal(outb[:T], out)
    assert torch.equal(outb[T:], ops.paged_prefill(q[:T2], kc, vc, full, 0,
                                                   window=W))


def test_model_prefill_sliding_window_matches_cpu():
    """smoke-llama, W = 48, 100 tokens: last-position logits against the
    fp32 CPU model on the same bf16 weights (relative 3e-2, the bound of
    test_model_prefill_paged_matches_cpu); the unwindowed model differs."""
    cfg = dataclasses.replace(get_config("smoke-llama"), sliding_window=48)
    m = build_model(cfg, dtype=torch.bfloat16, device=DEV, seed=11)
    cpu = build_model(cfg, dtype=torch.float32, seed=11)
    cpu.load_state_dict({k: v.float().cpu() for k, v in m.state_dict().items()})
    tok = torch.randint(1, 500, (1, 100), generator=torch.Generator().manual_seed(5))
    pos = torch.arange(100, dtype=torch.int32)
    ref = cpu.prefill(tok, pos, cpu.alloc_caches(8, "cpu"), pos)
    got = m.prefill(tok.to(DEV), pos.to(DEV), m.alloc_caches(8, DEV), pos.to(DEV))
    rel = (got.float().cpu() - ref).abs().max().item() / ref.abs().max().item()
    print(f"smoke-llama W=48 prefill: rel err {rel:.3e}")
    assert rel < 3e-2
    m = build_model("smoke-llama", dtype=torch.bfloat16, device=DEV, seed=11)
    full = m.prefill(tok.to(DEV), pos.to(DEV), m.alloc_caches(8, DEV), pos.to(DEV))
    assert not torch.equal(full, got)
