"""Batched (packed, "varlen") paged prefill on the GPU: the gfx950 kernel
flash_prefill_paged_batch (ops/csrc/attention_prefill_paged.hip) bit for
bit against the single-sequence kernel and against the fp32 reference,
its host checks, then the model and engine paths built on it."""
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


# (Hq, Hkv, dh, transposed-V, [(ctx, T) per sequence], pairs (a, b) where
# sequence b's first block IS sequence a's first block, as after a prefix hit)
BATCHES = [
    # the last sequence spans two tiles, the second ragged; a decode-shaped
    # row; a shared first block
    (8, 2, 128, True, [(0, 64), (48, 37), (16, 1), (272, 300)], [(1, 2)]),
    (4, 1, 64, False, [(100, 33), (0, 1), (40, 270)], []),
    (2, 2, 256, False, [(16, 1), (80, 40)], []),
    (2, 1, 256, True, [(0, 17), (31, 2)], []),
    (8, 2, 128, True, [(48, 37)], []),          # a batch of one
]


@pytest.mark.parametrize("Hq,Hkv,dh,vt,seqs,shared", BATCHES)
def test_paged_prefill_batch_kernel(Hq, Hkv, dh, vt, seqs, shared):
    assert ops.has_hip()
    torch.manual_seed(dh + 7 * len(seqs) + Hq)
    B = len(seqs)
    nbs = [(c + t + BS - 1) // BS for c, t in seqs]
    pool = sum(nbs) + 4
    perm = torch.randperm(pool).tolist()
    spare = perm.pop()
    maxb = max(nbs) + 2
    # every entry past a row's needed length points at the all-NaN spare
    table = torch.full((B, maxb), spare, dtype=torch.int32)
    kc, vc = ops.alloc_kv_cache(pool, Hkv, dh, DEV, v_transposed=vt)
    assert ops.attention._is_vt(kc, vc) == vt
    share_of = {b: a for a, b in shared}
    qs, ks, vs = [], [], []
    for b, (ctx, T) in enumerate(seqs):
        S = ctx + T
        blocks = [perm.pop() for _ in range(nbs[b])]
        k = torch.randn(S, Hkv, dh, dtype=torch.bfloat16, device=DEV)
        v = torch.randn(S, Hkv, dh, dtype=torch.bfloat16, device=DEV)
        pos = torch.arange(S)
        if b in share_of:
            a = share_of[b]
            blocks[0] = int(table[a, 0])
            k[:BS], v[:BS] = ks[a][:BS], vs[a][:BS]
            pos = pos[BS:]                       # block 0 is already written
        table[b, :nbs[b]] = torch.tensor(blocks, dtype=torch.int32)
        slots = (table[b][pos // BS].long() * BS + pos % BS).to(torch.int32)
        ops.kv_append(k[pos.to(DEV)], v[pos.to(DEV)], kc, vc, slots.to(DEV))
        qs.append(torch.randn(T, Hq, dh, dtype=torch.bfloat16, device=DEV))
        ks.append(k)
        vs.append(v)
    # whatever the kernel must not read is NaN: each last block's tail ...
    for b, (ctx, T) in enumerate(seqs):
        last, off = int(table[b, nbs[b] - 1]), (ctx + T) % BS
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
    q = torch.cat(qs)
    plan = ops.paged_prefill_plan([t for _, t in seqs], [c for c, _ in seqs],
                                  DEV)
    assert plan.ntiles == sum((t + 255) // 256 for _, t in seqs)

    out = ops.paged_prefill_batch(q, kc, vc, table_d, plan)
    torch.cuda.synchronize()
    assert out.shape == q.shape
    assert not torch.isnan(out.float()).any(), "stale cache contents leaked"

    lo = 0
    for b, (ctx, T) in enumerate(seqs):
        single = ops.paged_prefill(qs[b], kc, vc, table_d[b], ctx)
        nbad = int((out[lo:lo + T] != single).sum())
        print(f"  seq {b} ctx={ctx} T={T}: elements differing from "
              f"paged_prefill: {nbad}")
        assert torch.equal(out[lo:lo + T], single), \
            f"sequence {b}: {nbad} elements differ from paged_prefill"
        lo += T

    plan_c = ops.paged_prefill_plan(plan.q_lens, plan.ctx_lens, "cpu")
    ref = ops.paged_prefill_batch_ref(q.cpu().float(), kc.cpu().float(),
                                      vc.cpu().float(), table, plan_c)
    diff = (out.cpu().float() - ref).abs().max().item()
    print(f"paged_prefill_batch dh={dh} vt={vt} {seqs}: "
          f"max abs diff vs fp32 ref {diff:.3e}")
    assert diff < 3e-2, f"max diff {diff}"


def test_paged_prefill_batch_host_checks():
    """Inconsistent calls fail on the host, through the public op and
    through the extension entry point itself."""
    assert ops.has_hip()
    ext = ops.ext()
    kc, vc = ops.alloc_kv_cache(4, 2, 64, DEV)
    plan = ops.paged_prefill_plan([4, 20], [0, 16], DEV)     # needs 3 blocks
    q = torch.zeros(24, 2, 64, dtype=torch.bfloat16, device=DEV)
    bt = torch.zeros(2, 3, dtype=torch.int32, device=DEV)
    assert ops.paged_prefill_batch(q, kc, vc, bt, plan).shape == q.shape

    def both(q_, bt_, plan_):
        with pytest.raises((ValueError, RuntimeError)):
            ops.paged_prefill_batch(q_, kc, vc, bt_, plan_)
        with pytest.raises(RuntimeError):
            ext.flash_prefill_paged_batch(q_, kc, vc, bt_, plan_.dev,
                                          plan_.cpu, plan_.num_seqs, 0.125)

    both(q[:23].contiguous(), bt, plan)          # q rows != sum T_b
    both(q, bt[:, :2].contiguous(), plan)        # table narrower than needed
    both(q, bt[:1].contiguous(), plan)           # B: table 1, plan 2
    plan3 = ops.paged_prefill_plan([4, 19, 1], [0, 16, 0], DEV)
    both(q, bt, plan3)                           # B: table 2, plan 3
    # T_b = 0: no plan can be built ...
    with pytest.raises(ValueError):
        ops.paged_prefill_plan([4, 0], [0, 16], DEV)
    # ... and a hand-made one is refused: cu_q [0, 4, 4], ctx [0, 16], 1 tile
    bad = torch.tensor([0, 4, 4, 0, 16, 0, 0], dtype=torch.int32)
    with pytest.raises(RuntimeError):
        ext.flash_prefill_paged_batch(q[:4].contiguous(), kc, vc, bt,
                                      bad.to(DEV), bad, 2, 0.125)
    # a plan whose tile list does not match its lengths
    bad = plan.cpu.clone()
    bad[-1] = 256
    with pytest.raises(RuntimeError):
        ext.flash_prefill_paged_batch(q, kc, vc, bt, bad.to(DEV), bad, 2,
                                      0.125)
    # fp8 caches
    kc8, vc8 = ops.alloc_kv_cache(4, 2, 64, DEV, fp8=True)
    with pytest.raises((NotImplementedError, RuntimeError)):
        ops.paged_prefill_batch(q, kc8, vc8, bt, plan)
    with pytest.raises(RuntimeError):
        ext.flash_prefill_paged_batch(q, kc8, vc8, bt, plan.dev, plan.cpu, 2,
                                      0.125)
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", ["smoke-llama", "smoke-gemma"])
def test_model_prefill_paged_batch_matches_cpu(name):
    """prefill() of three prompts' prefixes (20, 0, 16 tokens), then ONE
    prefill_paged_batch over their tails (13, 9, 1) must give the logits of
    a one-pass fp32 prefill of each full prompt, and leave KV that
    paged_decode can use (relative 3e-2, as
    test_model_prefill_paged_matches_cpu)."""
    assert ops.has_hip()
    pre, tails = [20, 0, 16], [13, 9, 1]
    lens = [p + t for p, t in zip(pre, tails)]
    g = torch.Generator().manual_seed(5)
    prompts = [torch.randint(1, 500, (s,), generator=g).tolist()
               for s in lens]
    m = build_model(name, dtype=torch.bfloat16, device=DEV, seed=11)
    fuse_for_inference(m)
    cpu = build_model(name, dtype=torch.float32, seed=11)
    # share the exact bf16 weight values (see the gemma engine test)
    cpu.load_state_dict({k: v.float().cpu() for k, v in m.state_dict().items()})
    caches = m.alloc_caches(16, DEV)
    caches_c = cpu.alloc_caches(16, "cpu")
    rows = [[0, 1, 2], [3], [4, 5]]
    bt = torch.full((3, 3), 15, dtype=torch.int32)    # padding: never read
    for b, r in enumerate(rows):
        bt[b, :len(r)] = torch.tensor(r, dtype=torch.int32)

    def slots(b, lo, hi):
        return [rows[b][p // BS] * BS + p % BS for p in range(lo, hi)]

    def decode(model, caches, dev):
        t = torch.tensor([3, 4, 5], dtype=torch.long, device=dev)
        p = torch.tensor(lens, dtype=torch.int32, device=dev)
        sl = torch.tensor([slots(b, lens[b], lens[b] + 1)[0]
                           for b in range(3)], dtype=torch.int32, device=dev)
        seq = torch.tensor([s + 1 for s in lens], dtype=torch.int32,
                           device=dev)
        return model.decode(t, p, caches, sl, bt.to(dev), seq)

    def i32(x, dev):
        return torch.tensor(x, dtype=torch.int32, device=dev)

    with torch.no_grad():
        for b in range(3):
            if pre[b]:
                m.prefill(torch.tensor([prompts[b][:pre[b]]], device=DEV),
                          i32(list(range(pre[b])), DEV), caches,
                          i32(slots(b, 0, pre[b]), DEV))
        plan = ops.paged_prefill_plan(tails, pre, DEV)
        toks = sum((prompts[b][pre[b]:] for b in range(3)), [])
        pos = sum((list(range(pre[b], lens[b])) for b in range(3)), [])
        sl = sum((slots(b, pre[b], lens[b]) for b in range(3)), [])
        lp_g = m.prefill_paged_batch(
            torch.tensor(toks, dtype=torch.long, device=DEV), i32(pos, DEV),
            caches, i32(sl, DEV), bt.to(DEV), plan)
        ld_g = decode(m, caches, DEV)

        lp_c = torch.cat([
            cpu.prefill(torch.tensor([prompts[b]]),
                        i32(list(range(lens[b])), "cpu"), caches_c,
                        i32(slots(b, 0, lens[b]), "cpu"))
            for b in range(3)])
        ld_c = decode(cpu, caches_c, "cpu")
    assert lp_g.shape == lp_c.shape == (3, m.cfg.vocab_size)
    for what, got, ref in (("prefill_paged_batch", lp_g, lp_c),
                           ("decode", ld_g, ld_c)):
        got = got.float().cpu()
        for b in range(3):
            scale = ref[b].abs().max().item()
            rel = (got[b] - ref[b]).abs().max().item() / scale
            print(f"{name} {what} seq {b}: rel err {rel:.3e}")
            assert rel < 3e-2, (what, b, got[b, :8], ref[b, :8])


def test_engine_prefill_batch_gpu():
    """prefix hits skip compute inside a batched forward, tokens are valid
    and the pool ends clean."""
    assert ops.has_hip()
    m = build_model("smoke-llama", dtype=torch.bfloat16, seed=4)
    eng = Engine(m, device=DEV, kv_blocks=128, seed=11, prefix_cache=True,
                 prefill_from_cache=True, prefill_batch=4)
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
    assert eng.stats["prefill_batches"] >= 1
    assert eng.stats["prefill_batched_requests"] >= 2
    # the first request publishes; the other two are deferred by the
    # in-batch rule and hit
    assert eng.stats["prefix_skipped_tokens"] == 64
    assert eng.stats["prefill_tokens"] == 3 * 35 + 50 - 64
    eng.flush_prefix_cache()
    assert len(eng.allocator.free) == eng.allocator.num_blocks
