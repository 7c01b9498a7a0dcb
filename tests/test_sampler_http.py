"""top_k / min_p over the HTTP API (pattern: test_serve_http.py): both are
new request fields, honoured on a default engine."""
import pytest
import torch

from runbooks_amd.serve import Engine
from runbooks_amd.serve.http import build_app

fastapi = pytest.importorskip("fastapi")
from fastapi.testclient import TestClient  # noqa: E402


@pytest.fixture(scope="module")
def served():
    eng = Engine("tiny-llama", device="cpu", dtype=torch.float32,
                 kv_blocks=256, seed=7)
    app = build_app(eng, model_name="tiny-llama")
    with TestClient(app) as c:
        yield c, eng


def _text(client, path="/v1/completions", **body):
    if path.endswith("chat/completions"):
        payload = {"messages": [{"role": "user", "content": "hello"}],
                   "max_tokens": 6, **body}
    else:
        payload = {"prompt": "hello", "max_tokens": 6, **body}
    r = client.post(path, json=payload)
    assert r.status_code == 200, r.text
    c = r.json()["choices"][0]
    return c["text"] if "text" in c else c["message"]["content"]


def test_top_k_one_returns_the_greedy_completion(served):
    client, eng = served
    greedy = _text(client)
    before = eng.stats["sampler_batched_steps"]
    assert _text(client, top_k=1, temperature=1.0) == greedy
    assert eng.stats["sampler_batched_steps"] > before


def test_min_p_one_returns_the_greedy_completion(served):
    client, _ = served
    assert _text(client, min_p=1.0, temperature=1.0) == _text(client)


def test_chat_passes_top_k_and_min_p(served):
    client, eng = served
    path = "/v1/chat/completions"
    greedy = _text(client, path)
    before = eng.stats["sampler_batched_steps"]
    assert _text(client, path, top_k=1, temperature=1.0) == greedy
    assert _text(client, path, min_p=1.0, temperature=1.0) == greedy
    assert eng.stats["sampler_batched_steps"] > before


def test_top_k_filters_a_sampled_completion(served):
    """temperature 1 with top_k = 2: every token is one of the two most
    likely under the request's own logprobs."""
    client, _ = served
    r = client.post("/v1/completions",
                    json={"prompt": "abc", "max_tokens": 8, "top_k": 2,
                          "temperature": 1.0, "seed": 11, "logprobs": 2})
    assert r.status_code == 200, r.text
    lp = r.json()["choices"][0]["logprobs"]
    for tok_lp, top in zip(lp["token_logprobs"], lp["top_logprobs"]):
        assert tok_lp >= min(top.values()) - 1e-6
