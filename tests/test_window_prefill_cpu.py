"""Sliding-window prefill on the CPU: the reference ops and the model's
prefill against an explicit-mask float64 softmax."""
import dataclasses
import math

import pytest
import torch

from runbooks_amd import ops
from runbooks_amd.models import build_model, get_config
from runbooks_amd.ops.attention import causal_attention_ref


def attn64(q, k, v, window):
    """q [S, Hq, D], k / v [S, Hkv, D] -> float64 [S, Hq, D]: row p sees
    keys p - window < j <= p (window 0: every j <= p)."""
    S, g = q.shape[0], q.shape[1] // k.shape[1]
    k, v = (t.double().repeat_interleave(g, 1) for t in (k, v))
    s = torch.einsum("phd,jhd->hpj", q.double(), k) / math.sqrt(q.shape[2])
    d = torch.arange(S)[:, None] - torch.arange(S)[None]     # p - j
    s = s.masked_fill((d < 0) | (d >= (window or S)), float("-inf"))
    return torch.einsum("hpj,jhd->phd", torch.softmax(s, -1), v)


@pytest.mark.parametrize("vt", [False, True])
@pytest.mark.parametrize("W", [0, 1, 5, 37, 40])       # S = 37: S and S + 3
def test_refs_match_explicit_mask(W, vt):
    torch.manual_seed(W)
    S, ctx, BS = 37, 13, ops.BLOCK_SIZE
    q, k, v = torch.randn(S, 4, 16), torch.randn(S, 2, 16), torch.randn(S, 2, 16)
    want = attn64(q, k, v, W)
    # q_block 16: three chunks, the later ones start past the window's edge
    got = causal_attention_ref(q[None], k[None], v[None], q_block=16, window=W)
    assert (got[0] - want).abs().max().item() < 1e-5
    table = torch.randperm(6)[:3].to(torch.int32)
    kc, vc = ops.alloc_kv_cache(6, 2, 16, "cpu", dtype=torch.float32,
                                v_transposed=vt)
    pos = torch.arange(S)
    ops.kv_append_ref(k, v, kc, vc,
                      (table[pos // BS].long() * BS + pos % BS).int())
    plan = ops.paged_prefill_plan([S - ctx, S], [ctx, 0], "cpu")
    got = ops.paged_prefill_batch(torch.cat([q[ctx:], q]), kc, vc,
                                  table.repeat(2, 1), plan, window=W)
    assert (got - torch.cat([want[ctx:], want])).abs().max().item() < 1e-5
    assert torch.equal(got[:S - ctx], ops.paged_prefill(
        q[ctx:], kc, vc, table, ctx, window=W))
    if W == 0:      # no window: bit for bit the call without the parameter
        assert torch.equal(got[S - ctx:], ops.paged_prefill(q, kc, vc, table, 0))
        assert torch.equal(ops.flash_prefill(q[None], k[None], v[None], window=0),
                           causal_attention_ref(q[None], k[None], v[None]))


def test_model_prefill_honours_sliding_window(monkeypatch):
    """tiny-llama, W = 24, 40 tokens: prefill gives the logits of the
    no-cache forward run on the explicit-mask attention, not the unwindowed
    ones."""
    cfg = dataclasses.replace(get_config("tiny-llama"), sliding_window=24)
    m = build_model(cfg, dtype=torch.float32, seed=2)
    tok = torch.randint(1, 250, (1, 40), generator=torch.Generator().manual_seed(1))
    pos = torch.arange(40, dtype=torch.int32)
    got = m.prefill(tok, pos, m.alloc_caches(4, "cpu"), pos)
    with torch.no_grad():
        full = m(tok)[:, -1]
        monkeypatch.setattr(ops, "causal_attention", lambda q, k, v, scale: attn64(
            q[0], k[0], v[0], 24)[None].float())
        want = m(tok)[:, -1]
    tol = 1e-4 * want.abs().max().item()
    assert (got - want).abs().max().item() < tol
    assert (got - full).abs().max().item() > tol
