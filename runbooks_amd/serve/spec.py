"""Draft proposers for speculative decoding (Engine(speculative=K)).

A drafter is any object with ``propose(request, k) -> list[int]``: at most
``k`` tokens it expects to follow the request's prompt + output. The engine
verifies them in one forward (Transformer.verify) and keeps the ones the
sampler would have produced anyway, so a drafter only affects speed, never
the text. An optional ``forget(request_id)`` is called when a request
leaves the engine.
"""
from __future__ import annotations


class NgramDrafter:
    """Prompt-lookup ("n-gram") drafts from the request's own text: match
    the longest suffix, from ``n`` down to 1 tokens, of prompt + output
    against the earlier text and propose what followed the most recent
    match. Needs no model and costs a few dict operations per new token:
    per request it keeps, for each length m <= n, a map from every m-gram
    that has a successor to the index of its latest successor, extended by
    the tokens that arrived since the last call (never a rescan)."""

    def __init__(self, n: int = 3):
        if n < 1:
            raise ValueError(f"spec_ngram must be >= 1, got {n}")
        self.n = int(n)
        self._state: dict[int, dict] = {}

    def _index(self, request_id: int, hist: list[int]) -> dict:
        st = self._state.get(request_id)
        if st is None or st["len"] > len(hist) or \
                st["head"] != hist[:len(st["head"])]:
            # new request, or its text was rewritten: start over
            st = {"len": 0, "head": hist[:8],
                  "maps": [dict() for _ in range(self.n)]}
            self._state[request_id] = st
        maps = st["maps"]
        # token i is the successor of every gram that ends at i - 1
        for i in range(max(st["len"], 1), len(hist)):
            for m in range(1, min(self.n, i) + 1):
                maps[m - 1][tuple(hist[i - m:i])] = i
        st["len"] = len(hist)
        return st

    def propose(self, request, k: int) -> list[int]:
        if k <= 0:
            return []
        hist = request.prompt_ids + request.output_ids
        st = self._index(request.request_id, hist)
        for m in range(min(self.n, len(hist) - 1), 0, -1):
            i = st["maps"][m - 1].get(tuple(hist[-m:]))
            if i is not None:
                return hist[i:i + k]
        return []

    def forget(self, request_id: int) -> None:
        self._state.pop(request_id, None)
