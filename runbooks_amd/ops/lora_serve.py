"""Batched per-row LoRA for serving (csrc/lora_serve.hip).

A decode batch may mix rows that belong to different adapters and rows
with none: ``idx`` names, per activation row, a slot of preallocated
per-site stacks (serve/lora.py), -1 for no adapter.

  * ``a_stack`` [n_slots, S*R, K]: the S segments' ``lora_a`` (fused qkv
    3, fused gate-up 2, o/down 1) stacked along rows
  * ``b_stack`` [n_slots, N, R]: row n holds ``lora_b[n, :]`` of the
    segment that owns output column n
  * ``scales``  fp32 [n_slots]: alpha / r

GPU tensors run the gfx950 kernels (bf16 operands, fp32 ``t``); CPU
tensors run the fp32 PyTorch formulation below, any float dtype. The
wrappers check everything they can without waiting for the device; slot
values are checked only against ``idx_cpu`` when the caller has one (the
graphed decode validates them when it stages them), and the kernels
treat an out-of-range slot as "no adapter" rather than reading past the
stacks.
"""
from __future__ import annotations

import torch

from . import _backend

MAX_RANK = 64


def _check_rank(R: int, who: str) -> None:
    if R % 16 or not 16 <= R <= MAX_RANK:
        raise ValueError(f"{who}: pool rank must be a multiple of 16 and at "
                         f"most {MAX_RANK}, got {R}")


def _check_idx(idx, M: int, n_slots: int, idx_cpu, who: str) -> None:
    if idx.dtype != torch.int32 or idx.dim() != 1 or idx.shape[0] != M or \
            not idx.is_contiguous():
        raise ValueError(f"{who}: idx must be contiguous int32 [{M}], got "
                         f"{idx.dtype} {tuple(idx.shape)}")
    if idx_cpu is None and not idx.is_cuda:
        idx_cpu = idx
    if idx_cpu is not None:
        vals = idx_cpu.tolist() if isinstance(idx_cpu, torch.Tensor) \
            else list(idx_cpu)
        if len(vals) != M:
            raise ValueError(f"{who}: idx_cpu has {len(vals)} rows, idx {M}")
        for m, v in enumerate(vals):
            if not -1 <= v < n_slots:
                raise ValueError(f"{who}: idx[{m}] = {v} is not -1 or a slot "
                                 f"below {n_slots}")


def _check_seg_ends(seg_ends, N: int, who: str) -> tuple[int, ...]:
    ends = tuple(int(e) for e in seg_ends)
    if not 1 <= len(ends) <= 3 or ends[-1] != N or \
            any(b <= a for a, b in zip((0,) + ends, ends)):
        raise ValueError(f"{who}: seg_ends must be 1..3 ascending column "
                         f"ends, the last equal to N={N}; got {ends}")
    return ends


def lora_shrink(x: torch.Tensor, a_stack: torch.Tensor, idx: torch.Tensor,
                segments: int = 1, idx_cpu=None) -> torch.Tensor:
    """t [M, S*R] fp32 with t[m, j] = sum_k x[m, k] * a_stack[idx[m], j, k];
    a row with idx < 0 gets zeros. x is plain row-major [M, K]."""
    who = "lora_shrink"
    if x.dim() != 2 or a_stack.dim() != 3 or a_stack.shape[2] != x.shape[1]:
        raise ValueError(f"{who}: x [M, K] and a_stack [n_slots, S*R, K] "
                         f"expected, got {tuple(x.shape)} and "
                         f"{tuple(a_stack.shape)}")
    M, K = x.shape
    S = int(segments)
    if not 1 <= S <= 3 or a_stack.shape[1] % S:
        raise ValueError(f"{who}: segments must be 1..3 and divide a_stack's "
                         f"{a_stack.shape[1]} rows, got {S}")
    _check_rank(a_stack.shape[1] // S, who)
    if K % 8:
        raise ValueError(f"{who}: K must be a multiple of 8, got {K}")
    if x.dtype != a_stack.dtype or not x.is_contiguous() or \
            not a_stack.is_contiguous():
        raise ValueError(f"{who}: x and a_stack must be contiguous and of "
                         f"one dtype, got {x.dtype} and {a_stack.dtype}")
    _check_idx(idx, M, a_stack.shape[0], idx_cpu, who)
    if _backend.use_hip(x, a_stack, idx):
        if x.dtype != torch.bfloat16:
            raise ValueError(f"{who}: the gfx950 kernel takes bf16, got "
                             f"{x.dtype}")
        return _backend.ext().lora_shrink(x, a_stack, idx, S)
    return lora_shrink_ref(x, a_stack, idx)


def lora_shrink_ref(x, a_stack, idx):
    """fp32 PyTorch formulation: gather each row's stack, one bmm."""
    live = (idx >= 0)
    a = a_stack[idx.clamp_min(0).long()].float()          # [M, S*R, K]
    t = torch.bmm(a, x.float().unsqueeze(2)).squeeze(2)
    return t * live.unsqueeze(1).to(t.dtype)


def lora_expand_(y: torch.Tensor, t: torch.Tensor, b_stack: torch.Tensor,
                 scales: torch.Tensor, idx: torch.Tensor, seg_ends,
                 idx_cpu=None) -> torch.Tensor:
    """In place: y[m, n] += scales[idx[m]] * sum_j t[m, s*R + j] *
    b_stack[idx[m], n, j] for column n in segment s (``seg_ends``: 1..3
    ascending host ints, the last equal to N). Rows with idx < 0 are not
    written."""
    who = "lora_expand_"
    if y.dim() != 2 or t.dim() != 2 or b_stack.dim() != 3 or \
            scales.dim() != 1:
        raise ValueError(f"{who}: y [M, N], t [M, S*R], b_stack [n_slots, N, "
                         f"R], scales [n_slots] expected")
    M, N = y.shape
    ends = _check_seg_ends(seg_ends, N, who)
    R = b_stack.shape[2]
    _check_rank(R, who)
    if N % 8:
        raise ValueError(f"{who}: N must be a multiple of 8, got {N}")
    if b_stack.shape[1] != N or tuple(t.shape) != (M, len(ends) * R) or \
            scales.shape[0] != b_stack.shape[0]:
        raise ValueError(f"{who}: shapes do not agree: y {tuple(y.shape)}, "
                         f"t {tuple(t.shape)}, b_stack {tuple(b_stack.shape)}"
                         f", scales {tuple(scales.shape)}, {len(ends)} "
                         f"segments")
    if t.dtype != torch.float32 or scales.dtype != torch.float32 or \
            y.dtype != b_stack.dtype:
        raise ValueError(f"{who}: t and scales are fp32, y and b_stack share "
                         f"a dtype; got t {t.dtype}, scales {scales.dtype}, "
                         f"y {y.dtype}, b_stack {b_stack.dtype}")
    if not (y.is_contiguous() and t.is_contiguous() and
            b_stack.is_contiguous() and scales.is_contiguous()):
        raise ValueError(f"{who}: tensors must be contiguous")
    _check_idx(idx, M, b_stack.shape[0], idx_cpu, who)
    if _backend.use_hip(y, t, b_stack, idx):
        if y.dtype != torch.bfloat16:
            raise ValueError(f"{who}: the gfx950 kernel takes bf16 y, got "
                             f"{y.dtype}")
        return _backend.ext().lora_expand_(y, t, b_stack, scales, idx,
                                           list(ends))
    return lora_expand_ref_(y, t, b_stack, scales, idx, ends)


def lora_expand_ref_(y, t, b_stack, scales, idx, seg_ends):
    """fp32 PyTorch formulation, written back in y's dtype."""
    M, N = y.shape
    R = b_stack.shape[2]
    rows = torch.nonzero(idx >= 0).flatten()
    if rows.numel() == 0:
        return y
    slot = idx[rows].long()
    b = b_stack[slot].float()                               # [m, N, R]
    delta = torch.empty(rows.numel(), N, dtype=torch.float32,
                        device=y.device)
    lo = 0
    for s, hi in enumerate(seg_ends):
        ts = t[rows, s * R:(s + 1) * R]                     # [m, R]
        delta[:, lo:hi] = torch.bmm(b[:, lo:hi], ts.unsqueeze(2)).squeeze(2)
        lo = hi
    y[rows] = (y[rows].float() + scales[slot].unsqueeze(1) * delta) \
        .to(y.dtype)
    return y
