#!/usr/bin/env python3
"""Per-kernel microbenchmarks for the gfx950 HIP library.

Run on an MI355X box (one gpurun call):

    python benchmarks/kernels.py [--out gpurun_out/kernels.json]

Each row: kernel, shape, wall us (median of 30 after 10 warmup via CUDA
events), achieved GB/s against its minimal-traffic model, and the
speed-of-light fraction at 6.3 TB/s (the measured HBM rate,
MI355X_MICROARCH.md). Weight-streaming benches use FRESH tensors per
iteration so the 256 MB Infinity Cache cannot fake the rate.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from runbooks_amd import ops

HBM = 6.3e12  # achievable B/s


def timeit(fn, iters=30, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    start, end = torch.cuda.Event(True), torch.cuda.Event(True)
    for _ in range(iters):
        start.record()
        fn()
        end.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(end) * 1e3)  # us
    times.sort()
    return times[len(times) // 2]


def row(name, shape, us, bytes_moved, flops=0):
    gbs = bytes_moved / (us * 1e-6) / 1e9
    return {"kernel": name, "shape": shape, "us": round(us, 2),
            "GB/s": round(gbs, 1), "sol": round(gbs * 1e9 / HBM, 3),
            "TF/s": round(flops / (us * 1e-6) / 1e12, 1) if flops else None}


def report(out, args):
    for r in out:
        print(f"{r['kernel']:>22} {r['shape']:>16} {r['us']:>9.1f}us "
              f"{r['GB/s']:>7.1f} GB/s  sol={r['sol']:<5}"
              f" {('%.0f TF/s' % r['TF/s']) if r['TF/s'] else ''}"
              + (f"  F.linear {r['f_linear_bf16_us']:.1f}us ratio "
                 f"{r['ratio']}" if "ratio" in r else ""))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


def w4_gemm_rows(out, dev="cuda"):
    """csrc/gemm_w4.hip (int4 weight-only, any M) at the llama2-7b
    projection shapes for prefill-sized M, each against F.linear on the
    bf16 master (hipBLASLt, what these GEMMs run on without
    RB_W4_PREFILL / w4_resident) in the same process: the two are timed
    alternately, three rounds each, and the median round is reported.
    Three weights per shape are rotated. `ratio` = gemm_w4 / F.linear
    time (> 1: the int4 GEMM is slower)."""
    from runbooks_amd.ops.linear import _W4_REGISTRY, quantize_int4
    bf16 = torch.bfloat16
    for name, N, K in (("qkv", 12288, 4096), ("o_proj", 4096, 4096),
                       ("gate_up", 22016, 4096), ("down", 4096, 11008)):
        ws = [torch.randn(N, K, dtype=bf16, device=dev) * 0.02
              for _ in range(3)]
        q4 = [ops.ext().w4_swizzle(*quantize_int4(w)) for w in ws]
        _W4_REGISTRY.clear()
        for M in (128, 512, 2048):
            x = torch.randn(M, K, dtype=bf16, device=dev)
            i = [0]

            def g4():
                i[0] = (i[0] + 1) % 3
                return ops.ext().gemm_w4(x, *q4[i[0]], N, K)

            def lin():
                i[0] = (i[0] + 1) % 3
                return torch.nn.functional.linear(x, ws[i[0]])
            t4, tl = [], []
            for _ in range(3):
                t4.append(timeit(g4, iters=20, warmup=5))
                tl.append(timeit(lin, iters=20, warmup=5))
            us, ref = sorted(t4)[1], sorted(tl)[1]
            r = row(f"gemm_w4 {name}", f"{M}x{N}x{K}", us,
                    N * K // 2 + N * K // 64 * 2 + (M * K + M * N) * 2,
                    flops=2 * M * N * K)
            r["f_linear_bf16_us"] = round(ref, 2)
            r["ratio"] = round(us / ref, 2)
            out.append(r)
        del ws, q4


def dg_tail_rows(out, dev="cuda"):
    """decode_gemm / decode_gemm_w4 with the K tail through the ring
    (tail=1) against the one-step tail loop (tail=0), at the llama2-7b
    split-K shapes. down-proj (K = 11008, split 2: 86 k-steps per wave =
    80 ring + 6 tail) is the shape the ring tail is for; o_proj (32 steps
    per wave, no tail) is the control: a launch in which no wave has a
    tail runs the one-step-tail instantiation whatever `tail` says
    (dg_has_tail / w4_has_tail), so its two rows time the same binary and
    show the noise of the method. As for the decode norm above, each
    variant is captured as a graph of 40 launches over ten rotating
    weights (>= 335 MB, past the Infinity Cache) and the replays are timed
    alternately, three rounds; the median round is reported. The rows time
    the decode_gemm entry point, which at these splits also allocates the
    slabs and launches the combine kernel; the decode loop's down-proj
    goes through decode_gemm_raw and has neither. Both variants pay the
    same, so the difference is the kernel's; the absolute us and GB/s are
    not those of the kernel alone (profiles/README.md has them)."""
    from runbooks_amd.ops.linear import quantize_int4
    bf16 = torch.bfloat16
    e = ops.ext()
    for name, N, K in (("o_proj", 4096, 4096), ("down", 4096, 11008)):
        ws = [torch.randn(N, K, dtype=bf16, device=dev) * 0.02
              for _ in range(10)]
        sx = e.decode_swizzle_x(torch.randn(32, K, dtype=bf16, device=dev))
        sws = [e.decode_swizzle_w(w) for w in ws]
        n4 = 20 if K == 4096 else 10
        q4 = [e.w4_swizzle(*quantize_int4(ws[j % 10].roll(j // 10, 0)))
              for j in range(n4)]
        del ws
        variants = {
            "decode_gemm": (lambda j, t: e.decode_gemm(
                sx, sws[j % 10], 32, N, K, tail=t), N * K * 2),
            "decode_gemm_w4": (lambda j, t: e.decode_gemm_w4(
                sx, *q4[j % n4], 32, N, K, tail=t),
                N * K // 2 + N * K // 64 * 2),
        }
        for kern, (call, nbytes) in variants.items():
            graphs = {}
            for t in (0, 1):
                call(0, t)
                torch.cuda.synchronize()
                graphs[t] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graphs[t]):
                    for j in range(40):
                        call(j, t)
            us = {0: [], 1: []}
            for _ in range(3):
                for t in (0, 1):
                    us[t].append(timeit(graphs[t].replay, iters=20,
                                        warmup=5) / 40)
            for t in (0, 1):
                out.append(row(f"{kern} {name} tail={t}", f"32x{N}x{K}",
                               sorted(us[t])[1], nbytes,
                               flops=2 * 32 * N * K))
            del graphs
        del sws, q4


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=None)
    p.add_argument("--dg-tail-only", action="store_true",
                   help="only the decode GEMM ring-tail vs tail-loop rows")
    p.add_argument("--w4-gemm-only", action="store_true",
                   help="only the gemm_w4 vs F.linear rows")
    p.add_argument("--norm-only", action="store_true",
                   help="stop after the rmsnorm rows")
    args = p.parse_args()
    assert torch.cuda.is_available() and ops.has_hip()
    dev = "cuda"
    bf16 = torch.bfloat16
    out = []
    if args.w4_gemm_only:
        w4_gemm_rows(out, dev)
        return report(out, args)
    if args.dg_tail_only:
        dg_tail_rows(out, dev)
        return report(out, args)

    # rmsnorm fwd/bwd [2048, 4096]
    x = torch.randn(2048, 4096, dtype=bf16, device=dev)
    w = torch.randn(4096, dtype=bf16, device=dev)
    us = timeit(lambda: ops.rmsnorm(x, w, 1e-5))
    out.append(row("rmsnorm_fwd", "2048x4096", us, 2 * x.numel() * 2))
    y, inv = ops.ext().rmsnorm_fwd(x, w, 1e-5)
    dy = torch.randn_like(x)
    us = timeit(lambda: ops.ext().rmsnorm_bwd(x, w, dy, inv))
    out.append(row("rmsnorm_bwd", "2048x4096", us, 5 * x.numel() * 2))

    # decode norm, split-K slab variant at the llama2-7b decode shape:
    # rmsnorm_dec_kernel (default) vs the generic kernel (RB_DEC_NORM=0).
    # Eager calls of a ~5 us kernel time the host (7 us per call either
    # way), so each variant is captured as a graph of 50 launches, the way
    # the engine's decode step replays it, and the replay is timed.
    xd = torch.randn(32, 4096, dtype=bf16, device=dev)
    sd = torch.randn(2, 32, 4096, dtype=torch.float32, device=dev)
    dn_bytes = xd.numel() * 2 * 4 + sd.numel() * 4 + w.numel() * 2
    graphs = {}
    for knob in ("1", "0"):
        os.environ["RB_DEC_NORM"] = knob
        ops.ext().rmsnorm_res_slab_fwd_dec(xd, sd, w, 1e-5)
        torch.cuda.synchronize()
        graphs[knob] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[knob]):
            for _ in range(50):
                ops.ext().rmsnorm_res_slab_fwd_dec(xd, sd, w, 1e-5)
    del os.environ["RB_DEC_NORM"]
    for knob, name in (("1", "rmsnorm_dec_slab"),
                       ("0", "rmsnorm_dec_slab_generic")):
        us = timeit(graphs[knob].replay) / 50
        out.append(row(name, "32x4096 split2", us, dn_bytes))
    del graphs
    if args.norm_only:
        return report(out, args)

    # rope [2048, 32, 128]
    q = torch.randn(2048, 32, 128, dtype=bf16, device=dev)
    cos, sin = ops.rope_tables(128, 4096, device=dev)
    pos = torch.arange(2048, dtype=torch.int32, device=dev) % 512
    us = timeit(lambda: ops.rope(q, cos, sin, pos))
    out.append(row("rope_fwd", "2048x32x128", us, 2 * q.numel() * 2))

    # swiglu fwd [2048, 11008]
    g = torch.randn(2048, 11008, dtype=bf16, device=dev)
    u = torch.randn_like(g)
    us = timeit(lambda: ops.swiglu(g, u))
    out.append(row("swiglu_fwd", "2048x11008", us, 3 * g.numel() * 2))

    # packed GLU epilogues [2048, 2*11008] (swiglu validated; geglu gated)
    yp = torch.randn(2048, 2 * 11008, dtype=bf16, device=dev)
    us = timeit(lambda: ops.ext().swiglu_packed(yp))
    out.append(row("swiglu_packed", "2048x2x11008", us,
                   1.5 * yp.numel() * 2))
    us = timeit(lambda: ops.ext().geglu_packed(yp))
    out.append(row("geglu_packed", "2048x2x11008", us,
                   1.5 * yp.numel() * 2))

    # cross-entropy fwd+bwd [2048, 32000]
    logits = torch.randn(4, 512, 32000, dtype=bf16, device=dev,
                         requires_grad=True)
    tgt = torch.randint(0, 32000, (4, 512), device=dev)

    def ce():
        loss = ops.cross_entropy(logits, tgt)
        loss.backward()
        logits.grad = None
    us = timeit(ce)
    out.append(row("cross_entropy_fwd+bwd", "2048x32000", us,
                   3 * logits.numel() * 2))

    # batched per-request sampler [32, 32000]: top-p 0.9 on every row and
    # 5 logprobs; bytes = one read of the logits + the fp32 workspace
    # written once (its re-reads stay in L2)
    slog = torch.randn(32, 32000, device=dev).mul_(4).to(bf16)
    sparams, _ = ops.pack_sample_batch(
        [dict(temperature=0.8, top_p=0.9, seed=i) for i in range(32)])
    us = timeit(lambda: ops.sample_batch(slog, sparams, None, 5))
    out.append(row("sample_batch top_p L=5", "32x32000", us,
                   slog.numel() * (2 + 4)))

    # flash prefill / training fwd [4, 512, 32, 128]
    qq = torch.randn(4, 512, 32, 128, dtype=bf16, device=dev)
    kk, vv = torch.randn_like(qq), torch.randn_like(qq)
    fl = 4 * 4 * 32 * 512 * 512 * 128 / 2  # causal half
    us = timeit(lambda: ops.flash_prefill(qq, kk, vv))
    out.append(row("flash_prefill", "b4 s512 h32 d128", us,
                   4 * qq.numel() * 2, flops=fl))
    qg = qq.clone().requires_grad_(True)
    kg = kk.clone().requires_grad_(True)
    vg = vv.clone().requires_grad_(True)
    dyy = torch.randn_like(qq)

    def fabwd():
        o = ops.causal_attention(qg, kg, vg)
        o.backward(dyy)
        qg.grad = kg.grad = vg.grad = None
    us = timeit(fabwd, iters=15)
    out.append(row("flash_fwd+bwd", "b4 s512 h32 d128", us,
                   10 * qq.numel() * 2, flops=3.5 * fl))

    # prefill of a 128-token tail behind a 1024-token cached prefix, next to
    # the dense prefill of the whole 1152 tokens it replaces on a prefix hit
    CTX, TQ, HP = 1024, 128, 32
    SP = CTX + TQ
    qp = torch.randn(1, SP, HP, 128, dtype=bf16, device=dev)
    kp, vp = torch.randn_like(qp), torch.randn_like(qp)
    us = timeit(lambda: ops.flash_prefill(qp, kp, vp))
    out.append(row("flash_prefill", f"b1 s{SP} h{HP} d128", us,
                   4 * qp.numel() * 2, flops=4 * HP * SP * SP * 128 / 2))
    nbp = SP // 16
    btp = torch.randperm(nbp + 8, device=dev)[:nbp].to(torch.int32)
    slots = (btp.long().repeat_interleave(16) * 16 +
             torch.arange(SP, device=dev) % 16).to(torch.int32)
    qt = qp[0, CTX:].contiguous()
    flp = 4 * HP * 128 * (TQ * CTX + TQ * (TQ + 1) / 2)
    for vt in (False, True):
        kcp, vcp = ops.alloc_kv_cache(nbp + 8, HP, 128, dev, v_transposed=vt)
        ops.kv_append(kp[0], vp[0], kcp, vcp, slots)
        us = timeit(lambda: ops.paged_prefill(qt, kcp, vcp, btp, CTX))
        out.append(row("paged_prefill_vt" if vt else "paged_prefill",
                       f"ctx{CTX} T{TQ} h{HP} d128", us,
                       (2 * qt.numel() + 2 * SP * HP * 128) * 2, flops=flp))

    # paged decode b32 len512
    BS, B, L = 16, 32, 512
    nb = B * (L // BS) + 8
    kc = torch.randn(nb, 32, BS, 128, dtype=bf16, device=dev)
    vc = torch.randn_like(kc)
    bt = torch.arange(B * (L // BS), dtype=torch.int32,
                      device=dev).reshape(B, -1)
    sl = torch.full((B,), L, dtype=torch.int32, device=dev)
    qd = torch.randn(B, 32, 128, dtype=bf16, device=dev)
    us = timeit(lambda: ops.paged_decode(qd, kc, vc, bt, sl))
    out.append(row("paged_decode", f"b{B} len{L} h32 d128", us,
                   2 * B * 32 * L * 128 * 2))

    # gemma-width decode (Dh=256 instantiation; first validated round 2)
    kc2 = torch.randn(nb // 2, 16, BS, 256, dtype=bf16, device=dev)
    vc2 = torch.randn_like(kc2)
    bt2 = torch.arange(B // 2 * (L // BS), dtype=torch.int32,
                       device=dev).reshape(B // 2, -1)
    sl2 = torch.full((B // 2,), L, dtype=torch.int32, device=dev)
    qd2 = torch.randn(B // 2, 16, 256, dtype=bf16, device=dev)
    us = timeit(lambda: ops.paged_decode(qd2, kc2, vc2, bt2, sl2))
    out.append(row("paged_decode_dh256", f"b{B//2} len{L} h16 d256", us,
                   2 * (B // 2) * 16 * L * 256 * 2))

    # MFMA GQA decode (llama2-70b shape) over the transposed-V layout
    kc3 = torch.randn(nb, 8, BS, 128, dtype=bf16, device=dev)
    vc3 = torch.randn_like(kc3).permute(0, 1, 3, 2).contiguous()
    qd3 = torch.randn(B, 64, 128, dtype=bf16, device=dev)
    us = timeit(lambda: ops.paged_decode(qd3, kc3, vc3, bt, sl))
    out.append(row("paged_decode_mfma_gqa", f"b{B} len{L} 64/8 d128", us,
                   2 * B * 8 * L * 128 * 2))

    # MFMA LoRA B-merge vs the hipBLASLt K=16 accumulate
    yb = torch.randn(2048, 11008, dtype=bf16, device=dev)
    tb = torch.randn(2048, 16, dtype=bf16, device=dev)
    wb = torch.randn(11008, 16, dtype=bf16, device=dev)
    us = timeit(lambda: ops.ext().lora_badd_(yb, tb, wb, 2.0))
    out.append(row("lora_badd", "2048x11008 r16", us, 2 * yb.numel() * 2))
    us = timeit(lambda: yb.addmm_(tb, wb.t(), alpha=2.0))
    out.append(row("blaslt_lora_addmm", "2048x11008 r16", us,
                   2 * yb.numel() * 2))

    # decode GEMMs: fresh weights per call (no L3 reuse)
    from runbooks_amd.ops.linear import _W4_REGISTRY, quantize_int4
    for N, K in [(12288, 4096), (4096, 4096), (22016, 4096), (4096, 11008),
                 (32000, 4096)]:
        xs = torch.randn(32, K, dtype=bf16, device=dev)
        ws = [torch.randn(N, K, dtype=bf16, device=dev) for _ in range(10)]
        i = [0]

        def blas():
            i[0] = (i[0] + 1) % 10
            return xs @ ws[i[0]].t()
        us = timeit(blas)
        out.append(row(f"blaslt_decode", f"32x{N}x{K}", us, N * K * 2,
                       flops=2 * 32 * N * K))
        def skinny():
            i[0] = (i[0] + 1) % 10
            return ops.ext().skinny_gemm(xs, ws[i[0]])
        us = timeit(skinny)
        out.append(row(f"skinny_decode", f"32x{N}x{K}", us, N * K * 2,
                       flops=2 * 32 * N * K))
        # v2 weight-stream kernel over pre-swizzled operands (the
        # shipped decode path)
        sws = [ops.ext().decode_swizzle_w(w) for w in ws]
        sx = ops.ext().decode_swizzle_x(xs)

        def dgv2():
            i[0] = (i[0] + 1) % 10
            return ops.ext().decode_gemm(sx, sws[i[0]], 32, N, K)
        us = timeit(dgv2)
        out.append(row(f"decode_gemm_v2", f"32x{N}x{K}", us, N * K * 2,
                       flops=2 * 32 * N * K))
        del sws
        # the same GEMM with its consumer fused into the epilogue, on
        # the row-permuted layouts (llama2-7b: gate-up glu16, qkv rope16);
        # same 10-weight rotation as the rows above
        if (N, K) == (22016, 4096):
            sws = [ops.ext().decode_swizzle_w_layout(w, 1) for w in ws]

            def dgglu():
                i[0] = (i[0] + 1) % 10
                return ops.ext().decode_gemm_glu(sx, sws[i[0]], 32, N, K)
            us = timeit(dgglu)
            out.append(row("decode_gemm_swiglu", f"32x{N}x{K}", us,
                           N * K * 2, flops=2 * 32 * N * K))
            del sws
        if (N, K) == (12288, 4096):
            sws = [ops.ext().decode_swizzle_w_layout(w, 2, 32, 32, 128)
                   for w in ws]
            rc, rs = (t.to(dev) for t in ops.rope_tables(128, 4096, 10000.0))
            kcr, vcr = ops.alloc_kv_cache(64, 32, 128, dev)
            rpos = torch.arange(100, 132, dtype=torch.int32, device=dev)
            rslot = torch.arange(32, dtype=torch.int32, device=dev) * BS

            def dgrope():
                i[0] = (i[0] + 1) % 10
                return ops.ext().decode_gemm_rope_append(
                    sx, sws[i[0]], 32, N, K, rc, rs, rpos, kcr, vcr, rslot,
                    32)
            us = timeit(dgrope)
            out.append(row("decode_gemm_rope_append", f"32x{N}x{K}", us,
                           N * K * 2, flops=2 * 32 * N * K))
            del sws, kcr, vcr
        # int4 weight-only kernel (MODEL_LOAD_IN_4BIT): group-64 nibbles
        # + bf16 scales, same pre-swizzled x operand. 10 sets of 9-65 MB
        # would sit in the 256 MiB Infinity Cache, so rotate >= 600 MB.
        w4_bytes = N * K // 2 + N * K // 64 * 2
        n4 = max(10, -(-600_000_000 // w4_bytes))
        q4 = [ops.ext().w4_swizzle(*quantize_int4(
            ws[j] if j < 10 else
            torch.randn(N, K, dtype=bf16, device=dev))) for j in range(n4)]
        _W4_REGISTRY.clear()

        def dgw4():
            i[0] = (i[0] + 1) % n4
            return ops.ext().decode_gemm_w4(sx, *q4[i[0]], 32, N, K)
        us = timeit(dgw4)
        out.append(row(f"decode_gemm_w4", f"32x{N}x{K}", us,
                       N * K // 2 + N * K // 64 * 2,
                       flops=2 * 32 * N * K))
        del q4

    w4_gemm_rows(out, dev)
    dg_tail_rows(out, dev)

    # fp8 decode GEMM
    from runbooks_amd.ops.linear import quantize_fp8
    xs = torch.randn(32, 4096, dtype=bf16, device=dev)
    qs = [quantize_fp8(torch.randn(12288, 4096, dtype=bf16, device=dev))
          for _ in range(10)]
    i = [0]

    def fp8():
        i[0] = (i[0] + 1) % 10
        return ops.ext().skinny_gemm_fp8(xs, *qs[i[0]])
    us = timeit(fp8)
    out.append(row("skinny_fp8_decode", "32x12288x4096", us, 12288 * 4096,
                   flops=2 * 32 * 12288 * 4096))

    # train GEMM shapes (hipBLASLt, fresh weights)
    for M, N, K in [(2048, 4096, 4096), (2048, 11008, 4096),
                    (2048, 4096, 11008)]:
        xs = torch.randn(M, K, dtype=bf16, device=dev)
        ws = [torch.randn(N, K, dtype=bf16, device=dev) for _ in range(6)]
        i = [0]

        def tg():
            i[0] = (i[0] + 1) % 6
            return xs @ ws[i[0]].t()
        us = timeit(tg)
        out.append(row("blaslt_train", f"{M}x{N}x{K}", us,
                       (M * K + N * K + M * N) * 2, flops=2 * M * N * K))

    # fused AdamW multi-tensor: 224 LoRA-sized tensors
    ps = [torch.nn.Parameter(torch.randn(16 * 4096, dtype=bf16, device=dev))
          for _ in range(224)]
    opt = ops.FusedAdamW(ps, lr=1e-3)
    for pp in ps:
        pp.grad = torch.randn_like(pp)
    us = timeit(opt.step)
    total = sum(pp.numel() for pp in ps)
    out.append(row("adamw_multi_tensor", "224x64K", us, total * (2 + 2 + 16)))

    report(out, args)


if __name__ == "__main__":
    main()
