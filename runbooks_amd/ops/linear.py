"""Linear dispatch: route decode-shaped matmuls to the skinny GEMM.

Batch-<=32 single-token decode GEMMs are weight-bandwidth bound;
csrc/skinny_gemm.hip streams W at HBM rate where hipBLASLt's tiles
measured 25-45% (profiles/). Everything else (prefill, training) stays
on hipBLASLt via F.linear — the library is the right tool for big GEMMs.
"""
from __future__ import annotations

import os
import weakref

import torch
import torch.nn.functional as F

from . import _backend

# Round-1 tile kernel; superseded by decode_gemm (kept for A/B runs).
_USE_SKINNY = os.environ.get("RB_SKINNY_GEMM", "0") == "1"
# v2 weight-stream kernel (csrc/decode_gemm.hip): default-on; RB_DECODE_GEMM=0
# falls back to hipBLASLt.
_USE_DECODE_GEMM = os.environ.get("RB_DECODE_GEMM", "1") == "1"


# data_ptr(weight) -> (w8 uint8 view, f32 per-channel scale). Populated by
# quantize_fp8 (serving with MODEL_LOAD_IN_8BIT); looked up on the decode
# fast path.
_FP8_REGISTRY: dict[int, tuple[torch.Tensor, torch.Tensor]] = {}

# data_ptr(weight) -> fragment-lane-major copy ([N/32][K/16][lane][8])
# consumed by csrc/decode_gemm.hip. A second full-precision weight copy:
# 288 GB HBM3E per GPU makes layout-specialized decode weights the right
# trade on MI355X (prefill/training keep the original [N,K] tensor).
# value: (swizzled copy, (N, K), layout, weakref to the registered tensor).
# data_ptr alone is NOT a safe key — a freed weight's address gets
# recycled by later allocations, so every lookup verifies tensor
# identity through the weakref (stale entries are dropped lazily).
#
# layout = (tag, hq, hkv, dh) names the ROW ORDER of the swizzled copy
# (csrc/decode_gemm.hip LAYOUT_*): "plain"; "glu16" (fused gate-up: each
# 32-row block = 16 gate rows + the matching 16 up rows); "rope16" (fused
# qkv: each q/k block = 16 rows d + their rotate-half partners d + Dh/2).
# The permuted layouts let the GEMM epilogue apply SwiGLU/GeGLU or
# RoPE + KV append in place; every other caller gets y in the original
# column order through the kernel's un-permuting store. Only the swizzled
# copy is permuted — the [N, K] master is untouched.
_DECODE_W_REGISTRY: dict[int, tuple] = {}

_LAYOUT_ID = {"plain": 0, "glu16": 1, "rope16": 2}


def fused_epilogue_enabled() -> bool:
    """RB_FUSED_EPILOGUE=0 keeps the separate swiglu / qkv_rope_append
    kernels behind the decode GEMMs (A/B switch and test reference)."""
    return os.environ.get("RB_FUSED_EPILOGUE", "1") == "1"


def _registry_get(reg: dict, weight: torch.Tensor):
    if weight.device.type == "meta":     # released master: no storage to key
        return None
    entry = reg.get(weight.data_ptr())
    if entry is None:
        return None
    if entry[-1]() is not weight:
        del reg[weight.data_ptr()]
        return None
    return entry


def register_decode_weight(weight: torch.Tensor, layout: str = "plain",
                           hq: int = 0, hkv: int = 0, dh: int = 0) -> None:
    """Build + register the decode-GEMM weight layout for `weight`.
    `layout` "glu16" needs a fused gate-up [2I, K] with I % 16 == 0;
    "rope16" a fused qkv [(hq + 2*hkv) * dh, K] with (dh/2) % 16 == 0."""
    _check_master(weight, "the RB_DECODE_GEMM registration")
    for ptr in [p for p, e in _DECODE_W_REGISTRY.items() if e[-1]() is None]:
        del _DECODE_W_REGISTRY[ptr]          # purge dead entries
    if layout == "rope16":
        meta = (layout, int(hq), int(hkv), int(dh))
    else:
        meta = (layout, 0, 0, 0)
    ws = _backend.ext().decode_swizzle_w_layout(
        weight.data, _LAYOUT_ID[layout], *meta[1:])
    _DECODE_W_REGISTRY[weight.data_ptr()] = (
        ws, (int(weight.shape[0]), int(weight.shape[1])), meta,
        weakref.ref(weight))

E4M3_MAX = 448.0


@torch.no_grad()
def quantize_fp8(weight: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """Row-wise (per-output-channel) OCP e4m3 quantization; registers the
    pair so fast_linear dispatches to the fp8 decode GEMM. Pass the
    PERSISTENT tensor object (Parameter / fused buffer), not .data —
    lookups verify identity via weakref."""
    scale = weight.float().abs().amax(dim=1).clamp(min=1e-8) / E4M3_MAX
    w8 = (weight.float() / scale[:, None]).to(torch.float8_e4m3fn)
    w8_bytes = w8.view(torch.uint8).contiguous()
    _FP8_REGISTRY[weight.data_ptr()] = (w8_bytes, scale.contiguous(),
                                        weakref.ref(weight))
    return w8_bytes, scale


def dequantize_fp8(w8_bytes: torch.Tensor, scale: torch.Tensor,
                   dtype=torch.bfloat16) -> torch.Tensor:
    return (w8_bytes.view(torch.float8_e4m3fn).float() *
            scale[:, None]).to(dtype)


# data_ptr(weight) -> (wq_swz, sc_swz, (N, K), weakref to the registered
# tensor): the int4 kernel layout of csrc/decode_gemm_w4.hip. Populated by
# quantize_int4 (serving with MODEL_LOAD_IN_4BIT); same keying and
# weakref-identity rule as the registries above (see _registry_get).
_W4_REGISTRY: dict[int, tuple] = {}

W4_GROUP = 64

# id(placeholder) -> (wq_swz, sc_swz, (N, K), name, weakref to the
# placeholder): weights whose bf16 master release_w4_masters freed (int4-
# resident serving). The placeholder is a meta-device tensor of the
# master's shape and dtype, so it has no data_ptr to key on: these entries
# are keyed on object identity, verified through the weakref like the
# others. wq_swz / sc_swz are None for a released VIEW of a fused weight
# (q_proj.weight ...), which has no int4 copy of its own.
_W4_RELEASED: dict[int, tuple] = {}


def w4_prefill_enabled() -> bool:
    """RB_W4_PREFILL=1 sends M > 32 GEMMs on an int4-registered weight to
    csrc/gemm_w4.hip instead of F.linear on the bf16 master. Off by
    default; forced on while an int4-resident model is alive (its masters
    are gone)."""
    if os.environ.get("RB_W4_PREFILL", "0") == "1":
        return True
    if _W4_RELEASED:
        _purge_released()
    return bool(_W4_RELEASED)


def _released_get(weight: torch.Tensor):
    entry = _W4_RELEASED.get(id(weight))
    if entry is None or entry[-1]() is not weight:
        return None
    return entry


def _check_master(weight: torch.Tensor, what: str) -> None:
    """Raise instead of reading a released (placeholder) master."""
    if weight.device.type != "meta":
        return
    entry = _released_get(weight)
    name = entry[3] if entry is not None else "<unnamed>"
    raise RuntimeError(
        f"weight {name} {tuple(weight.shape)}: the model is int4-resident "
        f"(w4_resident), its bf16 master was released and {what} needs it. "
        "Only bf16, bias-free, no-grad inference runs on an int4-resident "
        "model")


def _w4_get(weight: torch.Tensor):
    """(wq_swz, sc_swz, (N, K), ...) of an int4-registered weight, released
    or not; None without one."""
    if weight.device.type == "meta":
        entry = _released_get(weight)
        return entry if entry is not None and entry[0] is not None else None
    if not _W4_REGISTRY:
        return None
    return _registry_get(_W4_REGISTRY, weight)


def _purge_released() -> None:
    for key in [k for k, e in _W4_RELEASED.items() if e[-1]() is None]:
        del _W4_RELEASED[key]


def w4_registered(weight: torch.Tensor) -> bool:
    """True when `weight` (released or not) has an int4 kernel copy."""
    return _w4_get(weight) is not None


def release_w4_placeholder(weight: torch.Tensor, name: str,
                           view: bool = False) -> torch.Tensor:
    """Meta-device stand-in for `weight` (same shape and dtype, no
    storage). The int4 registration of `weight` moves to the placeholder,
    keyed on identity; `view` marks a per-projection view of a fused
    weight, which has none of its own (and shares the fused weight's
    data_ptr, so it is not looked up). The caller swaps the placeholder in
    for every reference to `weight`; the master is freed when the last one
    goes."""
    _purge_released()
    entry = None if view else _registry_get(_W4_REGISTRY, weight)
    if entry is None and not view:
        raise RuntimeError(f"release_w4_placeholder: {name} has no int4 "
                           "registration")
    ph = torch.empty(weight.shape, dtype=weight.dtype, device="meta")
    if isinstance(weight, torch.nn.Parameter):
        ph = torch.nn.Parameter(ph, requires_grad=False)
    if entry is not None:
        del _W4_REGISTRY[weight.data_ptr()]
        _W4_RELEASED[id(ph)] = (entry[0], entry[1], entry[2], name,
                                weakref.ref(ph))
    else:
        _W4_RELEASED[id(ph)] = (None, None, tuple(weight.shape), name,
                                weakref.ref(ph))
    return ph


def _w4_codes(weight: torch.Tensor):
    if weight.dim() != 2 or weight.shape[1] % W4_GROUP != 0:
        raise ValueError(f"int4 quantization needs [N, K] with K % "
                         f"{W4_GROUP} == 0, got {tuple(weight.shape)}")
    n, k = weight.shape
    w =weight.detach().float().reshape(n, k // W4_GROUP, W4_GROUP)
    scales = (w.abs().amax(dim=2).clamp(min=1e-8) / 7).to(torch.bfloat16)
    codes = torch.round(w / scales.float()[:, :, None]).clamp_(-8, 7)
    return codes.reshape(n, k), scales


@torch.no_grad()
def quantize_int4(weight: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """Symmetric group-wise int4 along K (groups of 64): scale[n, g] =
    bf16(max(absmax, 1e-8) / 7), code = clamp(round(w / scale), -8, 7),
    stored nibble = code + 8. Returns the canonical pair: q uint8
    [N, K/2] (byte k/2 = even k in the low nibble, odd k in the high
    nibble) and scales bf16 [N, K/64].

    On a GPU tensor it also builds the decode kernel's layout
    (csrc/decode_gemm_w4.hip) and registers it so fast_linear dispatches
    to the int4 decode GEMM. Pass the PERSISTENT tensor object
    (Parameter / fused buffer), not .data — lookups verify identity via
    weakref."""
    codes, scales = _w4_codes(weight)
    nib = (codes + 8).to(torch.uint8)
    q = (nib[:, 0::2] | (nib[:, 1::2] << 4)).contiguous()
    scales = scales.contiguous()
    if _backend.use_hip(weight):
        ext = _backend.ext()
        n, k = int(weight.shape[0]), int(weight.shape[1])
        if ext.decode_gemm_w4_supported(32, n, k):
            for ptr in [p for p, e in _W4_REGISTRY.items()
                        if e[-1]() is None]:
                del _W4_REGISTRY[ptr]          # purge dead entries
            wq_swz, sc_swz = ext.w4_swizzle(q, scales)
            _W4_REGISTRY[weight.data_ptr()] = (wq_swz, sc_swz, (n, k),
                                               weakref.ref(weight))
    return q, scales


def dequantize_int4(q: torch.Tensor, scales: torch.Tensor,
                    dtype=torch.bfloat16) -> torch.Tensor:
    """(code * float(scale)).to(dtype) from the canonical pair. With
    dtype=bfloat16 (round-to-nearest-even) this is the exact weight the
    int4 decode kernel multiplies by."""
    n, kh = q.shape
    codes = torch.stack([q & 0xF, q >> 4], dim=2).reshape(n, 2 * kh)
    codes = codes.float() - 8.0
    w = codes.reshape(n, -1, W4_GROUP) * scales.float()[:, :, None]
    return w.reshape(n, 2 * kh).to(dtype)


@torch.no_grad()
def fake_quantize_int4_(weight: torch.Tensor) -> torch.Tensor:
    """In-place dequantize(quantize(w)); registers nothing. For tests and
    offline quality evaluation of the 4-bit format."""
    codes, scales = _w4_codes(weight)
    n, k = weight.shape
    w = codes.reshape(n, -1, W4_GROUP) * scales.float()[:, :, None]
    weight.copy_(w.reshape(n, k).to(weight.dtype))
    return weight


def gemm_w4(x: torch.Tensor, q4) -> torch.Tensor:
    """x [..., K] bf16 @ dequant(int4 entry q4)^T through csrc/gemm_w4.hip
    (any M; fast_linear uses it for M > 32)."""
    n, k = q4[2]
    y = _backend.ext().gemm_w4(x.reshape(-1, k).contiguous(), q4[0], q4[1],
                               n, k)
    return y.view(*x.shape[:-1], n)


def fast_linear(x: torch.Tensor, weight: torch.Tensor,
                bias: torch.Tensor | None = None) -> torch.Tensor:
    released = weight.device.type == "meta"
    if (bias is None and not torch.is_grad_enabled()
            and x.dtype == torch.bfloat16 and _backend.use_hip(x)
            and weight.is_contiguous()):
        k = x.shape[-1]
        m = x.numel() // k
        n = weight.shape[0]
        if m <= 32:
            if _W4_REGISTRY or released:
                q4 = _w4_get(weight)
                if q4 is not None and \
                        _backend.ext().decode_gemm_w4_supported(m, n, k):
                    # same operand contract as the bf16 v2 branch below
                    xs = getattr(x, "_rb_swz", None)
                    if xs is None:
                        xs = _backend.ext().decode_swizzle_x(
                            x.reshape(m, k).contiguous())
                    y = _backend.ext().decode_gemm_w4(xs, q4[0], q4[1],
                                                      m, n, k)
                    return y.view(*x.shape[:-1], n)
            if released:
                _check_master(weight, "a GEMM without an int4 kernel")
            if n % 64 == 0 and k % 256 == 0:
                q = _registry_get(_FP8_REGISTRY, weight)
                if q is not None:
                    y = _backend.ext().skinny_gemm_fp8(
                        x.reshape(m, k).contiguous(), q[0], q[1])
                    return y.view(*x.shape[:-1], n)
            if _USE_DECODE_GEMM:
                dw = _registry_get(_DECODE_W_REGISTRY, weight)
                if dw is not None:
                    # producers (rmsnorm_fwd_dec, *_packed_dec) attach the
                    # pre-swizzled operand; otherwise one tiny swizzle
                    # kernel builds it here
                    xs = getattr(x, "_rb_swz", None)
                    if xs is None:
                        xs = _backend.ext().decode_swizzle_x(
                            x.reshape(m, k).contiguous())
                    tag, hq, hkv, dh = dw[2]
                    y = _backend.ext().decode_gemm(
                        xs, dw[0], m, n, k, -1, _LAYOUT_ID[tag], hq, hkv, dh)
                    return y.view(*x.shape[:-1], n)
            if _USE_SKINNY and n % 64 == 0 and k % 256 == 0:
                y = _backend.ext().skinny_gemm(x.reshape(m, k).contiguous(),
                                               weight)
                return y.view(*x.shape[:-1], n)
        elif (_W4_REGISTRY or released) and w4_prefill_enabled():
            # int4 weight-only GEMM at large M: prefill, chunked and
            # batched prefill multiply by the weights decode streams
            q4 = _w4_get(weight)
            if q4 is not None and _backend.ext().gemm_w4_supported(m, n, k):
                return gemm_w4(x, q4)
    if released:
        _check_master(weight, "the F.linear path (non-bf16 input, bias, "
                      "grad enabled or CPU input)")
    return F.linear(x, weight, bias)


def decode_linear_raw(x, weight, xs=None, m=None):
    """Decode GEMM that may return an UNCOMBINED fp32 split-K slab
    [split, M, N] (consumer kernels fold it — rmsnorm_res_slab_fwd_dec),
    or a plain bf16 [M, N]. Falls back to fast_linear when the weight
    has no registered decode layout. Returns (out, is_slab).

    A producer that emits only the pre-swizzled operand (decode_linear_glu)
    passes it as `xs` with its row count `m` and x=None; the weight must
    then have a registered decode layout."""
    dw = _registry_get(_DECODE_W_REGISTRY, weight)
    if dw is None or not _USE_DECODE_GEMM:
        if x is None:
            raise RuntimeError("decode_linear_raw: operand-only input needs "
                               "a registered decode weight")
        with torch.no_grad():
            return fast_linear(x, weight), False
    k = weight.shape[1]
    n = weight.shape[0]
    if xs is None:
        m = x.numel() // k
        xs = getattr(x, "_rb_swz", None)
        if xs is None:
            xs = _backend.ext().decode_swizzle_x(x.reshape(m, k).contiguous())
    tag, hq, hkv, dh = dw[2]
    out = _backend.ext().decode_gemm_raw(xs, dw[0], m, n, k,
                                         _LAYOUT_ID[tag], hq, hkv, dh)
    return out, out.dtype == torch.float32


def decode_layout(weight) -> str | None:
    """Layout tag of `weight`'s registered decode copy (None: none)."""
    if not _USE_DECODE_GEMM:
        return None
    dw = _registry_get(_DECODE_W_REGISTRY, weight)
    return None if dw is None else dw[2][0]


def fused_epilogue_ok(x, weight, tag: str) -> bool:
    """True when the decode GEMM of x @ weight^T can run with the fused
    `tag` epilogue: matching registered layout, m <= 32, bf16, a
    single-pass (split == 1) GEMM, and RB_FUSED_EPILOGUE on."""
    if not (fused_epilogue_enabled() and x.dtype == torch.bfloat16
            and _backend.use_hip(x) and decode_layout(weight) == tag):
        return False
    k = x.shape[-1]
    n = weight.shape[0]
    ext = _backend.ext()
    return (x.numel() // k <= 32 and ext.decode_gemm_supported(
        x.numel() // k, n, k) and ext.decode_gemm_split(n, k) == 1)


def _operand(x, m, k):
    xs = getattr(x, "_rb_swz", None)
    if xs is None:
        xs = _backend.ext().decode_swizzle_x(x.reshape(m, k).contiguous())
    return xs


def decode_linear_glu(x, weight, gelu: bool = False):
    """Gate-up decode GEMM with SwiGLU (or GeGLU) fused into its epilogue
    (fused_epilogue_ok(x, weight, "glu16") must hold). Returns (operand,
    m): the down-proj decode operand, for decode_linear_raw(xs=, m=)."""
    dw = _registry_get(_DECODE_W_REGISTRY, weight)
    k = x.shape[-1]
    m = x.numel() // k
    return _backend.ext().decode_gemm_glu(
        _operand(x, m, k), dw[0], m, weight.shape[0], k, gelu), m


def decode_linear_rope_append(x, weight, cos, sin, positions, k_cache,
                              v_cache, slot_mapping, hq: int):
    """qkv decode GEMM with RoPE + paged KV append fused into its epilogue
    (fused_epilogue_ok(x, weight, "rope16") must hold; bf16 cache).
    Returns RoPE'd q [m, hq, dh]."""
    dw = _registry_get(_DECODE_W_REGISTRY, weight)
    if dw[2][1:] != (hq, k_cache.shape[1], k_cache.shape[3]):
        raise RuntimeError(f"decode_linear_rope_append: weight registered "
                           f"for heads {dw[2][1:]}, called with "
                           f"{(hq, k_cache.shape[1], k_cache.shape[3])}")
    k = x.shape[-1]
    m = x.numel() // k
    return _backend.ext().decode_gemm_rope_append(
        _operand(x, m, k), dw[0], m, weight.shape[0], k, cos, sin,
        positions, k_cache, v_cache, slot_mapping, hq)


class Linear(torch.nn.Linear):
    """nn.Linear with the decode-GEMM fast path."""

    def forward(self, x):
        return fast_linear(x, self.weight, self.bias)
