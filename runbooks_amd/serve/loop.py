"""The thread that steps the engine for the HTTP server.

Kept apart from serve/http.py so that it imports without the web framework:
it needs only the engine.
"""
from __future__ import annotations

import logging
import queue
import threading

from .engine import Engine

logger = logging.getLogger("runbooks_amd.serve")


class EngineLoop:
    """Background thread driving the continuous-batching engine."""

    def __init__(self, engine: Engine):
        self.engine = engine
        self._lock = threading.Lock()
        self._wake = threading.Event()
        self._watchers: dict[int, queue.Queue] = {}  # request_id -> token q
        self._failures = 0
        self._stop = False
        # calls that must run on the stepping thread, between steps
        # (adapter load / unload copy into memory the decode step reads)
        self._jobs: queue.Queue = queue.Queue()
        self._thread = threading.Thread(target=self._run, daemon=True)
        self._thread.start()

    def submit(self, prompt_ids, max_new_tokens, temperature,
               top_p=1.0, logprobs=None, seed=None,
               presence_penalty=0.0, frequency_penalty=0.0,
               repetition_penalty=1.0,
               stop_token_ids=(), top_k=0,
               min_p=0.0, adapter=None) -> tuple[queue.Queue, "object"]:
        """Returns (queue yielding token_id | None, engine Request)."""
        q: queue.Queue = queue.Queue()
        with self._lock:
            req = self.engine.submit(prompt_ids, max_new_tokens, temperature,
                                     top_p=top_p, logprobs=logprobs,
                                     seed=seed,
                                     presence_penalty=presence_penalty,
                                     frequency_penalty=frequency_penalty,
                                     repetition_penalty=repetition_penalty,
                                     stop_token_ids=stop_token_ids,
                                     top_k=top_k, min_p=min_p,
                                     **({} if adapter is None
                                        else {"adapter": adapter}))
            self._watchers[req.request_id] = q
            req._watch_sent = 0
        self._wake.set()
        return q, req

    def cancel(self, request_id: int) -> None:
        with self._lock:
            self.engine.cancel(request_id)

    def call(self, fn, timeout: float | None = 60.0):
        """Run fn() on the stepping thread between two steps and return
        its result (or raise what it raised)."""
        box: dict = {}
        done = threading.Event()
        self._jobs.put((fn, box, done))
        self._wake.set()
        if not done.wait(timeout):
            raise TimeoutError("engine loop did not run the call")
        if "error" in box:
            raise box["error"]
        return box.get("result")

    def load_adapter(self, name: str, path) -> None:
        """The file is read here, on the caller's thread and outside the
        lock, so submits and cancels are not held up by it; only the copy
        into the slot runs on the stepping thread."""
        from .lora import read_adapter
        state, alpha, r = read_adapter(path, self.engine.cfg)
        self.call(lambda: self.engine.load_adapter_state(name, state, alpha,
                                                         r))

    def unload_adapter(self, name: str) -> None:
        self.call(lambda: self.engine.unload_adapter(name))

    def _run_jobs(self) -> None:
        while True:
            try:
                fn, box, done = self._jobs.get_nowait()
            except queue.Empty:
                return
            with self._lock:
                try:
                    box["result"] = fn()
                except Exception as e:  # noqa: BLE001
                    box["error"] = e
            done.set()

    def _run(self):
        while not self._stop:
            self._run_jobs()
            if not self.engine.has_work():
                self._wake.wait(timeout=0.05)
                self._wake.clear()
                continue
            with self._lock:
                try:
                    finished = self.engine.step()
                    self._failures = 0
                except Exception:
                    # a rejected request is dropped from the queues —
                    # notify its watcher; on repeated failures (a request
                    # that keeps crashing the step) fail everything rather
                    # than spin
                    self._failures += 1
                    # a request part-way through a chunked prefill is in
                    # neither queue
                    pre = ([self.engine.prefilling]
                           if self.engine.prefilling is not None else [])
                    if self._failures >= 3:
                        for r in (self.engine.running +
                                  self.engine.waiting + pre):
                            r.finished = True
                            if r.blocks:
                                self.engine.allocator.release(r.blocks)
                                r.blocks = []
                        self.engine.running.clear()
                        self.engine.waiting.clear()
                        self.engine.prefilling = None
                        pre = []
                    alive = {r.request_id for r in
                             self.engine.running + self.engine.waiting + pre}
                    for rid in list(self._watchers):
                        if rid not in alive:
                            self._watchers.pop(rid).put(None)
                    continue
                live = list(self.engine.running) + finished
                for r in live:
                    q = self._watchers.get(r.request_id)
                    if q is None:
                        continue
                    sent = getattr(r, "_watch_sent", 0)
                    for t in r.output_ids[sent:]:
                        q.put(t)
                    r._watch_sent = len(r.output_ids)
                for r in finished:
                    q = self._watchers.pop(r.request_id, None)
                    if q is not None:
                        q.put(None)

    def shutdown(self):
        self._stop = True
        self._wake.set()
        self._thread.join(timeout=2)
        from ..utils.trace import dump_global
        p = dump_global()
        if p:
            logger.info("trace written to %s", p)
