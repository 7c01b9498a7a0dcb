"""Paged-cache prefill on the GPU: the gfx950 MFMA kernel
(ops/csrc/attention_prefill_paged.hip) against the fp32 reference and,
bit for bit, against flash_prefill on the concatenated sequence; then the
model and engine paths built on it."""
import pytest
import torch

from runbooks_amd import ops
from runbooks_amd.models import build_model
from runbooks_amd.models.transformer import fuse_for_inference
from runbooks_amd.serve import Engine

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BS = ops.BLOCK_SIZE
NAN = float("nan")


@pytest.mark.parametrize("ctx,T,Hq,Hkv,dh,vt", [
    (0, 64, 4, 4, 128, False),     # no prefix: one full LDS tile
    (48, 37, 8, 2, 128, True),     # GQA, ragged T, prefix not tile-aligned
    (272, 300, 4, 1, 64, False),   # MQA, two workgroups, many tiles
    (16, 1, 2, 2, 256, False),     # single query row, wide heads
    (100, 33, 8, 2, 64, True),     # ctx off the block grid, 2 waves
    (80, 40, 2, 1, 256, True),     # wide heads, transposed V, ctx off the tiles
    (40, 270, 2, 2, 128, False),   # prefix, two workgroups, the second ragged
])
def test_paged_prefill_kernel(ctx, T, Hq, Hkv, dh, vt):
    assert ops.has_hip()
    torch.manual_seed(ctx * 1000 + T)
    S = ctx + T
    q = torch.randn(S, Hq, dh, dtype=torch.bfloat16, device=DEV)
    k = torch.randn(S, Hkv, dh, dtype=torch.bfloat16, device=DEV)
    v = torch.randn(S, Hkv, dh, dtype=torch.bfloat16, device=DEV)

    # cache filled by kv_append through a shuffled, non-contiguous table
    nb = (S + BS - 1) // BS
    pool = nb + 4
    perm = torch.randperm(pool)
    spare = int(perm[nb])
    # trailing, unneeded entries point at a valid all-NaN spare block
    table = torch.cat([perm[:nb], torch.full((3,), spare)]).to(torch.int32)
    kc, vc = ops.alloc_kv_cache(pool, Hkv, dh, DEV, v_transposed=vt)
    assert ops.attention._is_vt(kc, vc) == vt
    pos = torch.arange(S)
    slots = (table[pos // BS].long() * BS + pos % BS).to(torch.int32)
    ops.kv_append(k, v, kc, vc, slots.to(DEV))
    # whatever the kernel must not read is NaN: the last block's tail ...
    last, off = int(table[nb - 1]), S % BS
    if off:
        kc[last, :, off:, :] = NAN
        if vt:
            vc[last, :, :, off:] = NAN
        else:
            vc[last, :, off:, :] = NAN
    # ... and the spare block
    kc[spare] = NAN
    vc[spare] = NAN
    table_d = table.to(DEV)

    out = ops.paged_prefill(q[ctx:], kc, vc, table_d, ctx)
    torch.cuda.synchronize()
    assert out.shape == (T, Hq, dh)
    assert not torch.isnan(out.float()).any(), "stale cache contents leaked"

    ref = ops.paged_prefill_ref(q[ctx:].cpu().float(), kc.cpu().float(),
                                vc.cpu().float(), table, ctx)
    diff = (out.cpu().float() - ref).abs().max().item()
    print(f"paged_prefill ctx={ctx} T={T} dh={dh} vt={vt}: "
          f"max abs diff vs fp32 ref {diff:.3e}")
    assert diff < 3e-2, f"max diff {diff}"

    dense = ops.flash_prefill(q[None], k[None], v[None])[0, ctx:]
    nbad = int((out != dense).sum())
    print(f"  elements differing from flash_prefill rows [ctx:]: {nbad}")
    assert torch.equal(out, dense), \
        f"{nbad} elements differ from flash_prefill on the concatenation"


def test_paged_prefill_rejects_fp8_cache():
    assert ops.has_hip()
    q = torch.zeros(4, 2, 64, dtype=torch.bfloat16, device=DEV)
    kc, vc = ops.alloc_kv_cache(2, 2, 64, DEV, fp8=True)
    bt = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises((NotImplementedError, RuntimeError)):
        ops.paged_prefill(q, kc, vc, bt, 0)
    with pytest.raises(RuntimeError):
        ops.ext().flash_prefill_paged(q, kc, vc, bt, 0, 0.125)


@pytest.mark.parametrize("name", ["smoke-llama", "smoke-gemma"])
def test_model_prefill_paged_matches_cpu(name):
    """prefill(20 tokens) then prefill_paged(next 13) must give the logits
    of a one-pass fp32 prefill of all 33, and leave KV that paged_decode
    can use (relative 3e-2, the bound of test_gemma_engine_decode_dh256)."""
    assert ops.has_hip()
    P, T = 20, 13
    S = P + T
    g = torch.Generator().manual_seed(5)
    prompt = torch.randint(1, 500, (S,), generator=g).tolist()
    m = build_model(name, dtype=torch.bfloat16, device=DEV, seed=11)
    fuse_for_inference(m)
    cpu = build_model(name, dtype=torch.float32, seed=11)
    # share the exact bf16 weight values (see the gemma engine test)
    cpu.load_state_dict({k: v.float().cpu() for k, v in m.state_dict().items()})
    caches = m.alloc_caches(8, DEV)
    caches_c = cpu.alloc_caches(8, "cpu")

    def tail(model, caches, dev):
        t = torch.tensor([3], dtype=torch.long, device=dev)
        p = torch.tensor([S], dtype=torch.int32, device=dev)
        bt = torch.tensor([[0, 1, 2]], dtype=torch.int32, device=dev)
        seq = torch.tensor([S + 1], dtype=torch.int32, device=dev)
        return model.decode(t, p, caches, p.clone(), bt, seq)

    with torch.no_grad():
        tok = torch.tensor([prompt], dtype=torch.long, device=DEV)
        pos = torch.arange(S, dtype=torch.int32, device=DEV)
        m.prefill(tok[:, :P], pos[:P], caches, pos[:P])
        bt = torch.tensor([0, 1, 2], dtype=torch.int32, device=DEV)
        lp_g = m.prefill_paged(tok[:, P:], pos[P:], caches, pos[P:], bt, P)
        ld_g = tail(m, caches, DEV)

        tok_c, pos_c = tok.cpu(), pos.cpu()
        lp_c = cpu.prefill(tok_c, pos_c, caches_c, pos_c)
        ld_c = tail(cpu, caches_c, "cpu")
    for what, got, ref in (("prefill_paged", lp_g, lp_c),
                           ("decode", ld_g, ld_c)):
        got = got.float().cpu()
        scale = ref.abs().max().item()
        rel = (got - ref).abs().max().item() / scale
        print(f"{name} {what}: rel err {rel:.3e}")
        assert rel < 3e-2, (what, got[:, :8], ref[:, :8])


def test_engine_paged_prefill_knobs_gpu():
    """Both knobs on: prefix hits skip compute, a long prompt is chunked,
    tokens are valid and the pool ends clean. (No token equality with the
    knobs-off engine: linears at M=3 and M=35 take different GEMMs.)"""
    assert ops.has_hip()
    m = build_model("smoke-llama", dtype=torch.bfloat16, seed=4)
    eng = Engine(m, device=DEV, kv_blocks=128, seed=11, prefix_cache=True,
                 prefill_from_cache=True, prefill_chunk=16)
    sys_prompt = list(range(1, 33))          # two full 16-token chunks
    reqs = [eng.submit(sys_prompt + [40 + i, 41 + i, 42 + i],
                       max_new_tokens=6) for i in range(3)]
    reqs.append(eng.submit([(i * 7 + 3) % 500 + 1 for i in range(50)],
                           max_new_tokens=6))
    for _ in range(200):
        if not eng.has_work():
            break
        eng.step()
    assert not eng.has_work()
    for r in reqs:
        assert r.finished and len(r.output_ids) == 6
        assert all(0 <= t < eng.cfg.vocab_size for t in r.output_ids)
    assert eng.stats["prefix_skipped_tokens"] == 64
    assert eng.stats["prefill_chunks"] > 0
    assert eng.stats["prefill_tokens"] == 3 * 35 + 50 - 64
    eng.flush_prefix_cache()
    assert len(eng.allocator.free) == eng.allocator.num_blocks
