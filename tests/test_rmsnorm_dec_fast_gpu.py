"""Decode norm fast path (rmsnorm_dec_kernel) against the generic
rmsnorm_fwd_kernel it replaces on the decode entry points: the two must
agree bit for bit, so RB_DEC_NORM=1 (default) is compared with
RB_DEC_NORM=0 by torch.equal on every output.

Bit-equality volume: 3 hidden sizes x 3 row counts x 5 modes x 3 seeds
compare (2048 + 4096 + 8192) * (1 + 5 + 32) = 544,768 elements per output
tensor and seed; 'none' has 2 output tensors (y, swz), the other four
modes 3 (sum, y, swz): 14 * 544,768 * 3 seeds = 22,880,256 outputs.
"""
import os

import pytest
import torch

from runbooks_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = 1e-5
SEEDS = (0, 1, 2)
ROWS = (1, 5, 32)
MODES = ("none", "res", "slab2", "slab4", "slab8")


class _knob:
    """RB_DEC_NORM for the calls inside the block (read per call)."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("RB_DEC_NORM")
        os.environ["RB_DEC_NORM"] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            del os.environ["RB_DEC_NORM"]
        else:
            os.environ["RB_DEC_NORM"] = self.old


def _bf16_tie_targets(shape, gen):
    """fp32 values within a few fp32 ulps of the midpoint between two
    neighbouring bf16 values: where a one-ulp change of the fp32 sum flips
    its bf16 rounding."""
    b = (torch.randn(shape, generator=gen, device=DEV) * 2.0).bfloat16()
    bits = b.view(torch.int16).to(torch.int32) << 16
    # midpoint = bf16 bits + half a bf16 ulp (0x8000), then -3..+3 fp32 ulps
    jitter = torch.randint(-3, 4, shape, generator=gen, device=DEV,
                           dtype=torch.int32)
    return (bits + 0x8000 + jitter).view(torch.float32)


def _inputs(mode, n_rows, D, seed):
    gen = torch.Generator(device=DEV).manual_seed(1000 * seed + D + n_rows)
    x = torch.randn(n_rows, D, generator=gen, device=DEV).bfloat16()
    w = (1.0 + 0.5 * torch.randn(D, generator=gen, device=DEV)).bfloat16()
    if mode == "none":
        return x, None, w
    if mode == "res":
        # same-exponent bf16 pairs: x + res needs 9 mantissa bits, so about
        # half the sums sit exactly on a bf16 tie
        res = torch.randn(n_rows, D, generator=gen, device=DEV).bfloat16()
        return x, res, w
    split = int(mode[4:])
    # slab slices of mixed magnitude: 1e-3 .. 10 per element
    mag = 10.0 ** (torch.rand(split, n_rows, D, generator=gen, device=DEV)
                   * 4.0 - 3.0)
    slabs = torch.randn(split, n_rows, D, generator=gen, device=DEV) * mag
    # on every second column, make slice 0 carry the total to a bf16 tie
    target = _bf16_tie_targets((n_rows, D), gen)
    rest = x.float() + slabs[1:].sum(0)
    tie = torch.arange(D, device=DEV) % 2 == 0
    slabs[0] = torch.where(tie, target - rest, slabs[0])
    return x, slabs.contiguous(), w


def _run(mode, x, extra, w, knob):
    ext = ops.ext()
    with _knob(knob):
        if mode == "none":
            y, swz = ext.rmsnorm_fwd_dec(x, w, EPS)
            return {"y": y, "swz": swz}
        if mode == "res":
            s, y, swz = ext.rmsnorm_res_fwd_dec(x, extra, w, EPS)
        else:
            s, y, swz = ext.rmsnorm_res_slab_fwd_dec(x, extra, w, EPS)
    return {"sum": s, "y": y, "swz": swz}


def _swz_rows(swz, n_rows, D):
    # [D/16][2][32][8]; rows >= n_rows are left uninitialised by design
    return swz.view(D // 16, 2, 32, 8)[:, :, :n_rows, :]


def _assert_same(fast, slow, n_rows, D, what):
    assert fast.keys() == slow.keys()
    n = 0
    for k in fast:
        a, b = fast[k], slow[k]
        if k == "swz":
            a, b = _swz_rows(a, n_rows, D), _swz_rows(b, n_rows, D)
        assert torch.equal(a, b), f"{what}: {k} differs"
        n += a.numel()
    return n


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("D", [2048, 4096, 8192])
def test_dec_norm_bit_equal(D, mode):
    assert ops.has_hip()
    n = 0
    for n_rows in ROWS:
        for seed in SEEDS:
            x, extra, w = _inputs(mode, n_rows, D, seed)
            fast = _run(mode, x, extra, w, "1")
            slow = _run(mode, x, extra, w, "0")
            n += _assert_same(fast, slow, n_rows, D,
                              f"D={D} rows={n_rows} {mode} seed={seed}")
    outs = 2 if mode == "none" else 3
    assert n == outs * D * sum(ROWS) * len(SEEDS)


def test_dec_norm_tie_inputs_hit_ties():
    """The slab inputs do what they claim: on the tie columns the fp32 sum
    lands within 16 fp32 ulps of a bf16 midpoint (the adds of the larger
    slices round at a coarser ulp than the target's, hence not within 3);
    a sum placed at random does so 33 times in 65536."""
    x, slabs, _ = _inputs("slab4", 5, 2048, 0)
    s = x.float()
    for sl in range(4):
        s = s + slabs[sl]
    low = s.view(torch.int32)[:, 0::2] & 0xFFFF
    near = ((low - 0x8000).abs() <= 16).float().mean().item()
    assert near > 0.9, near


@pytest.mark.parametrize("mode", MODES)
def test_dec_norm_fallback_shape(mode):
    """D = 5120 has no instantiation: both knob settings run the generic
    kernel, and it still matches the fp32 reference."""
    D, n_rows = 5120, 5
    x, extra, w = _inputs(mode, n_rows, D, 0)
    a = _run(mode, x, extra, w, "1")
    b = _run(mode, x, extra, w, "0")
    _assert_same(a, b, n_rows, D, f"fallback {mode}")
    _check_reference(mode, x, extra, w, a, n_rows, D)


def _check_reference(mode, x, extra, w, out, n_rows, D):
    s = x.float()
    if mode == "res":
        s = s + extra.float()
    elif mode != "none":
        for sl in range(extra.shape[0]):
            s = s + extra[sl]
    ref = ops.rmsnorm_ref(s, w.float(), EPS)
    tol = 2e-2      # tests/test_gpu_ops.py::test_rmsnorm_fwd, bf16
    assert torch.allclose(out["y"].float(), ref, atol=tol, rtol=tol)
    if mode != "none":
        # same fp32 adds in the same order, round-to-nearest-even: exact
        assert torch.equal(out["sum"], s.bfloat16())
    # swz is y in the decode GEMM's B-operand order
    assert torch.equal(_swz_rows(out["swz"], n_rows, D).permute(2, 0, 1, 3)
                       .reshape(n_rows, D), out["y"])


def test_dec_norm_reference():
    """Fast path against the plain-PyTorch fp32 reference, at the headline
    shape (32 rows, D=4096, two slab slices)."""
    D, n_rows = 4096, 32
    x, slabs, w = _inputs("slab2", n_rows, D, 0)
    out = _run("slab2", x, slabs, w, "1")
    _check_reference("slab2", x, slabs, w, out, n_rows, D)
