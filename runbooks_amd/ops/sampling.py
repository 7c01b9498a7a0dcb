"""Token sampling: greedy argmax / Gumbel-max temperature sampling."""
from __future__ import annotations

import torch

from . import _backend


def sample_tokens(logits: torch.Tensor, temperature: float = 0.0,
                  seed: int = 0, top_p: float = 1.0) -> torch.Tensor:
    """logits [..., V] -> int32 token ids [...]. temperature<=0 => greedy;
    0<top_p<1 applies nucleus filtering before sampling."""
    shape = logits.shape[:-1]
    flat = logits.reshape(-1, logits.shape[-1])
    if temperature > 0.0 and 0.0 < top_p < 1.0:
        flat = top_p_filter(flat.float(), top_p)
    if _backend.use_hip(logits):
        out = _backend.ext().sample_tokens(flat.contiguous(), float(temperature),
                                           int(seed))
        return out.reshape(shape)
    if temperature <= 0.0:
        return flat.argmax(dim=-1).to(torch.int32).reshape(shape)
    gen = torch.Generator(device="cpu").manual_seed(seed)
    u = torch.rand(flat.shape, generator=gen)
    g = -torch.log(-torch.log(u.clamp_min(1e-20)))
    return (flat.float() / temperature + g).argmax(dim=-1).to(torch.int32).reshape(shape)


def top_p_filter(logits: torch.Tensor, top_p: float) -> torch.Tensor:
    """Nucleus filtering: keep the smallest prefix of the sorted
    distribution with cumulative probability >= top_p; the rest -> -inf.
    Runs in torch (sampling happens OUTSIDE the decode hipGraph, so the
    sort here never lands in the captured stream)."""
    sorted_logits, idx = torch.sort(logits, dim=-1, descending=True)
    probs = torch.softmax(sorted_logits, dim=-1)
    cum = probs.cumsum(dim=-1)
    # shift so the token that crosses top_p stays included
    drop = cum - probs > top_p
    masked = sorted_logits.masked_fill(drop, float("-inf"))
    out = torch.full_like(logits, float("-inf"))
    return out.scatter(-1, idx, masked)


# ---------------------------------------------------------------------------
# Batched per-request sampler (csrc/sample_batch.hip)
# ---------------------------------------------------------------------------
# Per row: a = fp32 logits after penalties; logprobs describe a (no
# temperature, no filter). temperature <= 0 -> argmax(a), lowest id on
# ties. Otherwise z = a / temperature and each filter is a value threshold
# on z (ties at a threshold are all kept):
#   top_k > 0      keep z >= k-th largest z          (off when k >= V)
#   0 < top_p < 1  keep z >= the first value, walking the distinct values
#                  downward, at which the mass of {z >= value} within the
#                  softmax over the top-k survivors reaches top_p
#   min_p > 0      keep z >= zmax + ln(min_p)
# The token is the argmax over the kept set of z + Gumbel noise.

PARAM_WORDS = 10      # int32 words per packed row, floats bit-cast in place
OUT_FIXED = 4         # token, logprob, kept, thr
MAX_LOGPROBS = 20
_P_TEMP, _P_TOPK, _P_TOPP, _P_LNMINP, _P_PRES, _P_FREQ, _P_REP, _P_SEED_LO, \
    _P_SEED_HI = range(9)
_FLOAT_COLS = [_P_TEMP, _P_TOPP, _P_LNMINP, _P_PRES, _P_FREQ, _P_REP]


def _i32(x: int) -> int:
    """low 32 bits of x as a signed int32 value"""
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >= (1 << 31) else x


def pack_sample_batch(rows, counts=None):
    """Pack per-row sampling parameters (and the penalty token counts)
    into the two host buffers ``sample_batch`` takes.

    ``rows``: one mapping per row with any of ``temperature`` (0.0),
    ``top_k`` (0), ``top_p`` (1.0), ``min_p`` (0.0), ``presence`` (0.0),
    ``frequency`` (0.0), ``repetition`` (1.0), ``seed`` (0).
    ``counts``: per row, a ``{token id: count}`` mapping of the tokens
    seen so far, or None for a row without penalties.

    Returns ``(params, penalties)``: an int32 ``[B, PARAM_WORDS]`` CPU
    tensor, and the CSR ``[offsets(B+1) | ids | counts]`` as one int32 CPU
    vector, or None when no row carries counts."""
    import math
    B = len(rows)
    fl = torch.zeros(B, len(_FLOAT_COLS), dtype=torch.float32)
    params = torch.zeros(B, PARAM_WORDS, dtype=torch.int32)
    fvals, ivals = [], []
    for r in rows:
        min_p = float(r.get("min_p", 0.0))
        ln_min_p = (-math.inf if min_p <= 0.0
                    else math.log(min(min_p, 1.0)))
        fvals.append([float(r.get("temperature", 0.0)),
                      float(r.get("top_p", 1.0)), ln_min_p,
                      float(r.get("presence", 0.0)),
                      float(r.get("frequency", 0.0)),
                      float(r.get("repetition", 1.0))])
        seed = int(r.get("seed", 0)) & 0xFFFFFFFFFFFFFFFF
        ivals.append([max(0, min(int(r.get("top_k", 0)), 0x7FFFFFFF)),
                      _i32(seed), _i32(seed >> 32)])
    if B:
        fl = torch.tensor(fvals, dtype=torch.float32)
        params[:, _FLOAT_COLS] = fl.view(torch.int32)
        params[:, [_P_TOPK, _P_SEED_LO, _P_SEED_HI]] = torch.tensor(
            ivals, dtype=torch.int32)
    penalties = None
    if counts is not None and any(c for c in counts):
        assert len(counts) == B, "one counts entry per row"
        offsets, ids, cnts = [0], [], []
        for c in counts:
            if c:
                ids.extend(c.keys())
                cnts.extend(c.values())
            offsets.append(len(ids))
        penalties = torch.tensor(offsets + ids + cnts, dtype=torch.int32)
    return params, penalties


def _check_sample_batch(logits, params, penalties, num_logprobs):
    """Host-side validation, on the CPU copies only (no device sync).
    Returns (offsets, ids, counts) of the CSR, or None."""
    if logits.dim() != 2 or logits.shape[0] < 1 or logits.shape[1] < 1:
        raise ValueError("sample_batch: logits must be [B >= 1, V >= 1]")
    if logits.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError("sample_batch: logits must be bf16 or f32")
    if not logits.is_contiguous():
        raise ValueError("sample_batch: logits must be contiguous")
    B, V = logits.shape
    if not 0 <= int(num_logprobs) <= MAX_LOGPROBS:
        raise ValueError(
            f"sample_batch: num_logprobs must be in [0, {MAX_LOGPROBS}]")
    if (params.device.type != "cpu" or params.dtype != torch.int32
            or tuple(params.shape) != (B, PARAM_WORDS)
            or not params.is_contiguous()):
        raise ValueError("sample_batch: params must be a contiguous CPU "
                         f"int32 [B, {PARAM_WORDS}] tensor "
                         "(pack_sample_batch)")
    if penalties is None:
        return None
    if (penalties.device.type != "cpu" or penalties.dtype != torch.int32
            or penalties.dim() != 1 or not penalties.is_contiguous()):
        raise ValueError("sample_batch: penalties must be a contiguous CPU "
                         "int32 vector (pack_sample_batch)")
    rest = penalties.numel() - (B + 1)
    if rest < 0 or rest % 2:
        raise ValueError("sample_batch: penalty CSR size does not match "
                         "the batch")
    nnz = rest // 2
    off = penalties[:B + 1]
    ids = penalties[B + 1:B + 1 + nnz]
    cnt = penalties[B + 1 + nnz:]
    if int(off[0]) != 0 or int(off[-1]) != nnz or \
            bool((off[1:] < off[:-1]).any()):
        raise ValueError("sample_batch: bad CSR offsets")
    if nnz and (int(ids.min()) < 0 or int(ids.max()) >= V):
        raise ValueError(f"sample_batch: penalty id outside [0, {V})")
    if nnz and int(cnt.min()) < 0:
        raise ValueError("sample_batch: negative penalty count")
    return off, ids, cnt


class SampleBatchResult:
    """Outputs of ``sample_batch``: views of ONE packed int32 buffer
    ``raw`` [B, 4 + 2L] (floats bit-cast next to ints).

    ``tokens`` int32 [B]; ``logprobs`` f32 [B] (of the token, under a);
    ``kept`` int32 [B] (size of the kept set, V on greedy rows); ``thr``
    f32 [B] (final threshold on z, -inf when no filter is active);
    ``top_ids`` int32 [B, L] and ``top_logprobs`` f32 [B, L] (the L
    largest a, descending, ties by ascending id)."""

    def __init__(self, raw: torch.Tensor, num_logprobs: int):
        L = int(num_logprobs)
        assert raw.dtype == torch.int32 and raw.shape[1] == OUT_FIXED + 2 * L
        self.raw = raw
        self.num_logprobs = L
        f = raw.view(torch.float32)
        self.tokens = raw[:, 0]
        self.logprobs = f[:, 1]
        self.kept = raw[:, 2]
        self.thr = f[:, 3]
        self.top_ids = raw[:, OUT_FIXED:OUT_FIXED + L]
        self.top_logprobs = f[:, OUT_FIXED + L:OUT_FIXED + 2 * L]

    def host(self) -> "SampleBatchResult":
        """The same result on the CPU: one device-to-host copy."""
        if self.raw.device.type == "cpu":
            return self
        return SampleBatchResult(self.raw.cpu(), self.num_logprobs)


def sample_batch(logits: torch.Tensor, params: torch.Tensor,
                 penalties: torch.Tensor | None = None,
                 num_logprobs: int = 0) -> SampleBatchResult:
    """Sample one token per row of ``logits`` [B, V] with per-row
    parameters: penalties, temperature, top-k / top-p / min-p, seeded
    draw, the token's logprob and the top ``num_logprobs`` logprobs.
    ``params`` / ``penalties`` come from ``pack_sample_batch``. On the GPU
    this is one kernel launch; ``.host()`` on the result is the one
    download. CPU tensors run ``sample_batch_ref`` with a generator per
    row seeded from that row's seed (reproducible and independent of the
    batch, but not the GPU's tokens)."""
    if _backend.use_hip(logits):
        _check_sample_batch(logits, params, penalties, num_logprobs)
        raw = _backend.ext().sample_batch(logits, params, penalties,
                                          int(num_logprobs))
        return SampleBatchResult(raw, num_logprobs)
    return sample_batch_ref(logits, params, penalties, num_logprobs)


def gumbel_from_uniform(u: torch.Tensor) -> torch.Tensor:
    return -torch.log(-torch.log(u.clamp_min(1e-20)))


def sample_batch_ref(logits: torch.Tensor, params: torch.Tensor,
                     penalties: torch.Tensor | None = None,
                     num_logprobs: int = 0, noise: torch.Tensor | None = None,
                     generator: torch.Generator | None = None
                     ) -> SampleBatchResult:
    """Plain-torch reference of the sampler semantics (fp32 values, fp64
    masses and log-sum-exp), row by row, on the CPU copy of ``logits``.

    ``noise`` [B, V] is added to z before the argmax (Gumbel noise for a
    real draw, zeros to test the filters alone); otherwise ``generator``
    draws it; otherwise each row draws from a generator seeded with its
    own packed seed. The result also carries ``adjusted`` (a, fp32
    [B, V])."""
    x = logits.detach().cpu()
    csr = _check_sample_batch(x, params, penalties, num_logprobs)
    B, V = x.shape
    L = int(num_logprobs)
    pf = params.view(torch.float32)
    raw = torch.zeros(B, OUT_FIXED + 2 * L, dtype=torch.int32)
    res = SampleBatchResult(raw, L)
    adjusted = torch.empty(B, V, dtype=torch.float32)
    if noise is not None:
        noise = noise.detach().cpu().float()
        assert tuple(noise.shape) == (B, V)
    elif generator is not None:
        noise = gumbel_from_uniform(torch.rand(B, V, generator=generator))
    ninf = float("-inf")
    for b in range(B):
        a = x[b].float().clone()
        if csr is not None:
            off, ids, cnt = csr
            s, e = int(off[b]), int(off[b + 1])
            if e > s:
                # the exact expression of Engine._apply_penalties
                idl = ids[s:e].long()
                c = cnt[s:e].float()
                a[idl] -= float(pf[b, _P_FREQ]) * c + float(pf[b, _P_PRES])
                rep = float(pf[b, _P_REP])
                if rep != 1.0:
                    seen = a[idl]
                    a[idl] = torch.where(seen > 0, seen / rep, seen * rep)
        adjusted[b] = a
        a64 = a.double()
        lse = torch.logsumexp(a64, dim=-1)
        order = torch.sort(a, descending=True, stable=True).indices
        temp = pf[b, _P_TEMP]
        tok = int(order[0])            # argmax, lowest id on ties
        kept, thr = V, ninf
        if float(temp) > 0.0:
            z = a / temp               # fp32
            zmax = z.max()
            thr_t = torch.tensor(ninf)
            keep = torch.ones(V, dtype=torch.bool)
            k = int(params[b, _P_TOPK])
            if 0 < k < V:
                thr_t = torch.maximum(thr_t, torch.topk(z, k).values[-1])
                keep = z >= thr_t
            top_p = float(pf[b, _P_TOPP])
            if 0.0 < top_p < 1.0:
                zs = torch.sort(z[keep], descending=True).values
                mass = torch.exp(zs.double() - zmax.double())
                cum = mass.cumsum(0)
                j = int(torch.searchsorted(cum, top_p * float(cum[-1])))
                thr_t = torch.maximum(thr_t, zs[min(j, zs.numel() - 1)])
            ln_min_p = pf[b, _P_LNMINP]
            if float(ln_min_p) != ninf:
                thr_t = torch.maximum(thr_t, zmax + ln_min_p)
            keep = z >= thr_t
            kept, thr = int(keep.sum()), float(thr_t)
            if noise is not None:
                g = noise[b]
            else:
                seed = (int(params[b, _P_SEED_LO]) & 0xFFFFFFFF) | (
                    (int(params[b, _P_SEED_HI]) & 0xFFFFFFFF) << 32)
                gen = torch.Generator(device="cpu").manual_seed(seed)
                g = gumbel_from_uniform(torch.rand(V, generator=gen))
            score = torch.where(keep, z + g, torch.tensor(ninf))
            best = score.max()
            tok = int((score == best).nonzero()[0]) if bool(keep.any()) \
                else tok
        raw[b, 0] = tok
        res.logprobs[b] = float(a64[tok] - lse)
        raw[b, 2] = kept
        res.thr[b] = thr
        n = min(L, V)
        if L:
            res.top_ids[b, :n] = order[:n].int()
            res.top_ids[b, n:] = -1
            res.top_logprobs[b, :n] = (a64[order[:n]] - lse).float()
            res.top_logprobs[b, n:] = ninf
    res.adjusted = adjusted
    return res
