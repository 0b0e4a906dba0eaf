"""OpenAI API server: schema, SSE streaming, stop strings, health/metrics/models
(CPU engine with a tiny random model)."""
import json
import os

import pytest
from fastapi.testclient import TestClient

from kubernetes_gpu_cluster_amd.engine.config import EngineConfig
from kubernetes_gpu_cluster_amd.entrypoints.api_server import build_app
from kubernetes_gpu_cluster_amd.entrypoints.async_engine import AsyncLLMEngine
from kubernetes_gpu_cluster_amd.utils.tokenizer import get_tokenizer


def _cfg():
    return EngineConfig(model="tiny-llama", random_init=True, max_model_len=256, max_num_seqs=8,
                        max_num_batched_tokens=128, device="cpu", dtype="float32")


@pytest.fixture(scope="module", params=["thread", "core-process"])
def client(request):
    cfg = _cfg()
    if request.param == "thread":
        eng = AsyncLLMEngine(cfg)
    else:
        from kubernetes_gpu_cluster_amd.entrypoints.engine_core import EngineCoreClient
        eng = EngineCoreClient(cfg)
    tok = get_tokenizer(cfg.model, eng.engine.mcfg)
    app = build_app(eng, tok, "tiny-llama", eng.engine.max_model_len)
    with TestClient(app) as c:
        yield c
    eng.shutdown()


def test_models_health_metrics(client):
    r = client.get("/v1/models")
    assert r.status_code == 200 and r.json()["data"][0]["id"] == "tiny-llama"
    assert client.get("/health").text == "ok"
    assert client.get("/ping").status_code == 200 and client.post("/ping").status_code == 200
    assert r.json()["data"][0]["root"] == "tiny-llama"
    client.post("/v1/completions", json={"prompt": "hi", "max_tokens": 2})
    m = client.get("/metrics").text
    assert "vllm:generation_tokens_total" in m and "vllm:time_to_first_token_seconds" in m


def test_completion(client):
    r = client.post("/v1/completions", json={"prompt": "hello world", "max_tokens": 7,
                                             "temperature": 0, "ignore_eos": True})
    j = r.json()
    assert r.status_code == 200, j
    assert j["object"] == "text_completion"
    assert j["usage"]["completion_tokens"] == 7
    assert j["choices"][0]["finish_reason"] == "length"
    # token-id prompt + seeded sampling is reproducible
    body = {"prompt": [5, 6, 7, 8], "max_tokens": 5, "seed": 11, "ignore_eos": True}
    a = client.post("/v1/completions", json=body).json()["choices"][0]["text"]
    b = client.post("/v1/completions", json=body).json()["choices"][0]["text"]
    assert a == b


def test_chat_and_stream(client):
    r = client.post("/v1/chat/completions", json={
        "messages": [{"role": "user", "content": "hi"}], "max_tokens": 4, "ignore_eos": True})
    j = r.json()
    assert j["object"] == "chat.completion" and j["choices"][0]["message"]["role"] == "assistant"
    with client.stream("POST", "/v1/chat/completions", json={
            "messages": [{"role": "user", "content": "hi"}], "max_tokens": 6, "stream": True,
            "ignore_eos": True}) as s:
        lines = [l for l in s.iter_lines() if l]
    assert lines[-1] == "data: [DONE]"
    chunks = [json.loads(l[6:]) for l in lines[:-1]]
    assert chunks[0]["choices"][0]["delta"].get("role") == "assistant"
    assert chunks[-1]["choices"][0]["finish_reason"] == "length"


def test_errors(client):
    r = client.post("/v1/completions", json={"prompt": "x" * 600, "max_tokens": 2})
    assert r.status_code == 400
    r = client.post("/v1/completions", json={"prompt": "x", "temperature": -1})
    assert r.status_code == 400
    r = client.post("/v1/completions", json={"prompt": "x", "n": 0})
    assert r.status_code == 400


class _ByteTok:
    """ids are UTF-8 bytes; decode like a byte-level BPE (invalid tails -> U+FFFD)."""

    def decode(self, ids):
        return bytes(ids).decode("utf-8", errors="replace")


def test_incremental_detok_matches_full_decode():
    from kubernetes_gpu_cluster_amd.entrypoints.api_server import _Detok
    text = "héllo wörld — ünïcode ✓ end"
    ids = list(text.encode())
    d = _Detok(_ByteTok(), [])
    out = "".join(d.update(ids[:i]) for i in range(1, len(ids) + 1)) + d.flush()
    assert out == text == d.text
    d2 = _Detok(_ByteTok(), ["zz", "longer-stop"])   # holdback, no stop hit
    out2 = "".join(d2.update(ids[:i]) for i in range(1, len(ids) + 1)) + d2.flush()
    assert out2 == text and not d2.stopped


def test_incremental_detok_stop_straddles_updates():
    from kubernetes_gpu_cluster_amd.entrypoints.api_server import _Detok
    ids = list("abc STOP def".encode())
    d = _Detok(_ByteTok(), ["STOP"])
    out = "".join(d.update(ids[:i]) for i in range(1, len(ids) + 1))
    assert d.stopped and out == "abc " and d.text == "abc "


def test_engine_core_death_is_reported():
    """The engine-core process dies -> /health 503 (pod restart) and requests fail fast."""
    from kubernetes_gpu_cluster_amd.entrypoints.engine_core import EngineCoreClient
    eng = EngineCoreClient(_cfg())
    tok = get_tokenizer("tiny-llama", eng.mcfg)
    app = build_app(eng, tok, "tiny-llama", eng.max_model_len)
    with TestClient(app) as c:
        assert c.get("/health").status_code == 200
        assert c.post("/v1/completions", json={"prompt": [5, 6], "max_tokens": 2}).status_code == 200
        eng._proc.kill()
        eng._proc.join(10)
        import time
        for _ in range(50):
            if not eng.is_alive:
                break
            time.sleep(0.1)
        assert c.get("/health").status_code == 503
        r = c.post("/v1/completions", json={"prompt": [5, 6], "max_tokens": 2})
        assert r.status_code == 503
    eng.shutdown()


def test_completion_logprobs(client):
    r = client.post("/v1/completions", json={"prompt": [5, 6, 7], "max_tokens": 4, "logprobs": 3,
                                             "temperature": 0, "ignore_eos": True})
    lp = r.json()["choices"][0]["logprobs"]
    assert len(lp["tokens"]) == 4 and len(lp["token_logprobs"]) == 4
    for v, top in zip(lp["token_logprobs"], lp["top_logprobs"]):
        assert v <= 0 and 1 <= len(top) <= 3
        # greedy: the chosen token is the most likely one (token strings may collide in
        # the legacy dict format, so compare against the listed maxima)
        assert v >= max(top.values()) - 1e-4
    assert lp["text_offset"] == sorted(lp["text_offset"])
    assert client.post("/v1/completions", json={"prompt": "x", "logprobs": 99}).status_code == 400


def test_chat_logprobs_stream(client):
    with client.stream("POST", "/v1/chat/completions", json={
            "messages": [{"role": "user", "content": "hi"}], "max_tokens": 3, "stream": True,
            "ignore_eos": True, "logprobs": True, "top_logprobs": 2}) as s:
        lines = [l for l in s.iter_lines() if l and l != "data: [DONE]"]
    content = [c for l in lines for c in (json.loads(l[6:])["choices"][0].get("logprobs") or {}).get("content", [])]
    assert len(content) == 3
    assert all(len(c["top_logprobs"]) == 2 and c["logprob"] <= 0 for c in content)


def test_n_choices_and_penalties(client):
    r = client.post("/v1/completions", json={"prompt": [5, 6, 7], "max_tokens": 4, "n": 3,
                                             "seed": 7, "ignore_eos": True,
                                             "presence_penalty": 0.5, "frequency_penalty": 0.2,
                                             "logit_bias": {"9": 2.0}, "min_p": 0.01})
    j = r.json()
    assert r.status_code == 200, j
    assert [c["index"] for c in j["choices"]] == [0, 1, 2]
    assert j["usage"]["completion_tokens"] == 12
    with client.stream("POST", "/v1/chat/completions", json={
            "messages": [{"role": "user", "content": "hi"}], "max_tokens": 3, "n": 2,
            "stream": True, "ignore_eos": True}) as s:
        lines = [l for l in s.iter_lines() if l and l != "data: [DONE]"]
    idx = {json.loads(l[6:])["choices"][0]["index"] for l in lines}
    assert idx == {0, 1}
    assert client.post("/v1/completions", json={"prompt": "x", "n": 99}).status_code == 400
    assert client.post("/v1/completions", json={"prompt": "x", "presence_penalty": 5}).status_code == 400


def test_shared_core_serves_two_frontends(request):
    """--api-server-count: one engine core, two attached frontends; each frontend gets
    exactly its own requests' outputs, and a detached frontend leaves the core running."""
    import asyncio

    from kubernetes_gpu_cluster_amd.engine.sequence import SamplingParams
    from kubernetes_gpu_cluster_amd.entrypoints.engine_core import EngineCoreClient, start_core
    cfg = _cfg()
    # sun_path holds ~107 bytes and pytest's tmp_path (base temp + user + test name) can
    # exceed that: keep the socket in a short directory of its own, as the server does
    # (api_server.py: mkdtemp(prefix="kgc-core-")), falling back to /tmp for a deep TMPDIR
    import shutil
    import tempfile
    sock_dir = tempfile.mkdtemp(prefix="kgc-core-")
    if len(os.path.join(sock_dir, "core.sock").encode()) > 100:
        shutil.rmtree(sock_dir, ignore_errors=True)
        sock_dir = tempfile.mkdtemp(prefix="kgc-core-", dir="/tmp")
    request.addfinalizer(lambda: shutil.rmtree(sock_dir, ignore_errors=True))
    addr, key = os.path.join(sock_dir, "core.sock"), b"k" * 32
    core = start_core(cfg, addr, key, 2)
    a = EngineCoreClient(cfg, connect=(addr, key), core_proc=core)
    b = EngineCoreClient(cfg, connect=(addr, key))
    sp = SamplingParams(max_tokens=5, ignore_eos=True, temperature=0.0)

    async def run(cl, rid, prompt):
        toks = []
        async for o in cl.generate(prompt, sp, rid):
            toks = list(o.output_token_ids)
        return toks

    async def go():
        return await asyncio.gather(run(a, "a1", [5, 6, 7]), run(b, "b1", [5, 6, 7]),
                                    run(a, "a2", [8, 9]), run(b, "b2", [8, 9]))
    ra1, rb1, ra2, rb2 = asyncio.run(go())
    assert len(ra1) == 5 and ra1 == rb1 and ra2 == rb2
    b.shutdown()                       # detach one frontend; the core keeps serving
    assert asyncio.run(run(a, "a3", [5, 6, 7])) == ra1
    a.shutdown()
    core.join(30)
    assert not core.is_alive()


def test_tokenize_detokenize(client):
    """vLLM's /tokenize (prompt or chat messages) and /detokenize round trip."""
    r = client.post("/tokenize", json={"prompt": "hello world"})
    j = r.json()
    assert r.status_code == 200, j
    assert j["count"] == len(j["tokens"]) > 0 and j["max_model_len"] == 256
    d = client.post("/detokenize", json={"tokens": j["tokens"]})
    assert d.status_code == 200 and "hello world" in d.json()["prompt"]
    c = client.post("/tokenize", json={"messages": [{"role": "user", "content": "hi"}]})
    assert c.status_code == 200 and c.json()["count"] > 0
    assert client.post("/tokenize", json={}).status_code == 400
    assert client.post("/detokenize", json={"tokens": [10 ** 9]}).status_code == 400


def test_api_key_guards_v1_routes():
    """--api-key (vLLM semantics): /v1 routes need the bearer token, probes stay open."""
    cfg = _cfg()
    eng = AsyncLLMEngine(cfg)
    try:
        tok = get_tokenizer(cfg.model, eng.engine.mcfg)
        app = build_app(eng, tok, "tiny-llama", eng.engine.max_model_len, api_key="s3cret")
        with TestClient(app) as c:
            assert c.get("/v1/models").status_code == 401
            assert c.get("/v1/models", headers={"Authorization": "Bearer nope"}).status_code == 401
            ok = c.get("/v1/models", headers={"Authorization": "Bearer s3cret"})
            assert ok.status_code == 200 and ok.json()["data"][0]["id"] == "tiny-llama"
            r = c.post("/v1/completions", json={"prompt": "hi", "max_tokens": 2},
                       headers={"Authorization": "Bearer s3cret"})
            assert r.status_code == 200
            assert c.get("/health").status_code == 200
            assert c.get("/metrics").status_code == 200
    finally:
        eng.shutdown()


def test_batched_prompts(client):
    """A list of prompts in one completions request: choice index = prompt * n + choice,
    echo per prompt, usage summed; streamed chunks carry every index and end in [DONE]."""
    body = {"prompt": ["hello", "world peace"], "max_tokens": 3, "n": 2, "ignore_eos": True,
            "temperature": 0, "echo": True}
    r = client.post("/v1/completions", json=body)
    j = r.json()
    assert r.status_code == 200, j
    assert [c["index"] for c in j["choices"]] == [0, 1, 2, 3]
    assert j["choices"][0]["text"].startswith("hello")
    assert j["choices"][0]["text"] == j["choices"][1]["text"]       # greedy: same per prompt
    assert j["usage"]["completion_tokens"] == 12
    single = client.post("/v1/completions", json=dict(body, prompt="hello", n=1)).json()
    assert single["choices"][0]["text"] == j["choices"][0]["text"]
    r = client.post("/v1/completions", json=dict(body, stream=True, echo=False))
    events = [l[6:] for l in r.text.splitlines() if l.startswith("data: ")]
    assert events[-1] == "[DONE]"
    seen = {json.loads(e)["choices"][0]["index"] for e in events[:-1]}
    assert seen == {0, 1, 2, 3}
    # token-id prompts batch the same way
    r = client.post("/v1/completions", json={"prompt": [[5, 6, 7], [8, 9]], "max_tokens": 2})
    assert r.status_code == 200 and [c["index"] for c in r.json()["choices"]] == [0, 1]


def test_stream_include_usage(client):
    """stream_options.include_usage: one usage event (no choices) right before [DONE]."""
    for path, body in (("/v1/completions", {"prompt": [5, 6, 7]}),
                       ("/v1/chat/completions", {"messages": [{"role": "user", "content": "hi"}]})):
        for n in (1, 2):
            r = client.post(path, json=dict(body, max_tokens=3, n=n, ignore_eos=True, stream=True,
                                            stream_options={"include_usage": True}))
            events = [l[6:] for l in r.text.splitlines() if l.startswith("data: ")]
            assert events[-1] == "[DONE]"
            u = json.loads(events[-2])
            assert u["choices"] == [] and u["usage"]["completion_tokens"] == 3 * n
            assert all("usage" not in json.loads(e) for e in events[:-2])


def test_stream_finalizer_takes_no_lock():
    """A stream finalizer can run in the middle of EngineCoreClient._send (a cyclic GC pass
    while pickling a message, on the thread that holds _send_lock): __del__ must not take
    that lock (it would deadlock the event loop).  The abort is recorded lock-free and
    sent from a normal context afterwards."""
    import asyncio
    import gc
    from kubernetes_gpu_cluster_amd.engine.sequence import SamplingParams
    from kubernetes_gpu_cluster_amd.entrypoints.engine_core import EngineCoreClient
    eng = EngineCoreClient(_cfg())

    async def body():
        g = eng.generate([5, 6, 7], SamplingParams(max_tokens=200, ignore_eos=True), "drop-2")
        with eng._send_lock:          # as if the GC ran inside _send on this thread
            del g
            gc.collect()              # returns: the finalizer only queued the abort
        for _ in range(100):          # the scheduled drain sends it
            if not eng._dropped:
                break
            await asyncio.sleep(0.02)
        assert not eng._dropped
    try:
        asyncio.run(asyncio.wait_for(body(), 30))
    finally:
        eng.shutdown()


@pytest.mark.parametrize("kind", ["thread", "core-process"])
def test_unstarted_stream_aborts_request(kind):
    """A request submitted eagerly whose output stream is dropped before the first chunk
    is read (client gone before the response starts) is aborted in the engine instead of
    decoding to max_tokens in a batch slot nobody reads."""
    import asyncio
    import gc
    import time
    from kubernetes_gpu_cluster_amd.engine.sequence import SamplingParams
    cfg = _cfg()
    if kind == "thread":
        eng = AsyncLLMEngine(cfg)
    else:
        from kubernetes_gpu_cluster_amd.entrypoints.engine_core import EngineCoreClient
        eng = EngineCoreClient(cfg)

    async def submit_and_drop():
        g = eng.generate([5, 6, 7], SamplingParams(max_tokens=200, ignore_eos=True), "drop-1")
        del g
        gc.collect()
        # a finished request's stream closes without an abort
        g2 = eng.generate([5, 6], SamplingParams(max_tokens=2, ignore_eos=True), "keep-1")
        outs = [o async for o in g2]
        assert outs[-1].finished and len(outs[-1].output_token_ids) == 2

    try:
        asyncio.run(submit_and_drop())
        # wait until the engine goes idle (step count stable), then: the dropped request
        # never finished (an unaborted one would have run to its 200 tokens)
        last, stable = -1, 0
        for _ in range(200):
            st = asyncio.run(eng.engine_stats())
            stable = stable + 1 if st["steps"] == last else 0
            last = st["steps"]
            if stable >= 5:
                break
            time.sleep(0.05)
        assert stable >= 5, "engine never went idle"
        assert all(r[3] != 200 for r in st["requests"]), st["requests"]
        assert any(r[3] == 2 for r in st["requests"])
        if kind == "thread":
            assert "drop-1" not in eng.engine.seqs
    finally:
        eng.shutdown()


@pytest.mark.parametrize("kind", ["thread", "core-process"])
def test_finished_request_is_logged_before_its_stream_ends(kind):
    """bench.py's engine-side window reads /kgc/engine_stats right after the client's last
    [DONE]: every request whose stream has ended must already be in the engine's done log
    (the thread engine once pushed a step's outputs before logging them, and under CPU load
    the last request of a wave fell out of the window)."""
    import asyncio
    from kubernetes_gpu_cluster_amd.engine.sequence import SamplingParams
    cfg = _cfg()
    if kind == "thread":
        eng = AsyncLLMEngine(cfg)
        # make the race deterministic: the step's outputs stall before the log would be
        # written on the old order, so a late log is visible to the check below
        orig = eng._push_step

        def push_then_check(outs):
            orig(outs)
            import time as _t
            _t.sleep(0.05)
        eng._push_step = push_then_check
    else:
        from kubernetes_gpu_cluster_amd.entrypoints.engine_core import EngineCoreClient
        eng = EngineCoreClient(cfg)

    async def body():
        for i in range(3):
            g = eng.generate([5, 6, 7 + i], SamplingParams(max_tokens=3, ignore_eos=True),
                             f"log-{i}")
            outs = [o async for o in g]
            assert outs[-1].finished
            st = await eng.engine_stats()
            assert sum(1 for r in st["requests"] if r[3] == 3) == i + 1, st["requests"]
    try:
        asyncio.run(asyncio.wait_for(body(), 60))
    finally:
        eng.shutdown()
