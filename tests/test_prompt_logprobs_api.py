"""prompt_logprobs and echo + logprobs through the OpenAI API server (CPU engine, tiny random
model; the engine in a thread and in the engine-core process)."""
import json

import pytest
from fastapi.testclient import TestClient

from kubernetes_gpu_cluster_amd.engine.config import EngineConfig
from kubernetes_gpu_cluster_amd.entrypoints.api_server import build_app
from kubernetes_gpu_cluster_amd.entrypoints.async_engine import AsyncLLMEngine
from kubernetes_gpu_cluster_amd.utils.tokenizer import get_tokenizer

PROMPT = [5, 6, 7, 8, 9]


@pytest.fixture(scope="module", params=["thread", "core-process"])
def served(request):
    cfg = EngineConfig(model="tiny-llama", random_init=True, max_model_len=256, max_num_seqs=8,
                       max_num_batched_tokens=128, device="cpu", dtype="float32")
    if request.param == "thread":
        eng = AsyncLLMEngine(cfg)
    else:
        from kubernetes_gpu_cluster_amd.entrypoints.engine_core import EngineCoreClient
        eng = EngineCoreClient(cfg)
    tok = get_tokenizer(cfg.model, eng.engine.mcfg)
    asked = []                                   # prompt_logprobs of every engine request
    generate = eng.generate

    def recording(ids, params, rid):
        asked.append(params.prompt_logprobs)
        return generate(ids, params, rid)
    eng.generate = recording
    app = build_app(eng, tok, "tiny-llama", eng.engine.max_model_len)
    with TestClient(app) as c:
        yield c, asked, tok
    eng.shutdown()


def _post(c, path, **body):
    r = c.post(path, json=body)
    assert r.status_code == 200, r.text
    return r.json()


def _check_plp(plp, ids, n):
    assert isinstance(plp, list) and len(plp) == len(ids) and plp[0] is None
    for t, e in zip(ids[1:], plp[1:]):
        assert str(t) in e and n <= len(e) <= n + 1
        for v in e.values():
            assert v["logprob"] <= 0 and isinstance(v["decoded_token"], str)
        others = [v["logprob"] for k, v in e.items() if k != str(t)]
        assert len(e) == n + 1 or e[str(t)]["logprob"] >= min(others, default=0)


def test_echo_logprobs_cover_the_prompt(served):
    c, asked, tok = served
    del asked[:]
    j = _post(c, "/v1/completions", prompt=PROMPT, echo=True, logprobs=2, max_tokens=3,
              temperature=0, ignore_eos=True)
    ch = j["choices"][0]
    lp = ch["logprobs"]
    assert len(lp["tokens"]) == len(lp["token_logprobs"]) == len(lp["top_logprobs"]) == \
        len(lp["text_offset"]) == 8
    assert lp["token_logprobs"][0] is None and lp["top_logprobs"][0] is None
    assert all(v <= 0 for v in lp["token_logprobs"][1:])
    assert all(isinstance(t, dict) and 1 <= len(t) <= 2 for t in lp["top_logprobs"][1:])
    assert lp["text_offset"][0] == 0 and lp["text_offset"] == sorted(lp["text_offset"])
    assert "".join(lp["tokens"]) == ch["text"]
    assert lp["tokens"][:5] == [tok.decode([t]) for t in PROMPT]
    assert "prompt_logprobs" not in ch and asked == [2]
    # the generated part is what the request without echo returns
    k = _post(c, "/v1/completions", prompt=PROMPT, logprobs=2, max_tokens=3, temperature=0,
              ignore_eos=True)["choices"][0]["logprobs"]
    assert lp["tokens"][5:] == k["tokens"] and len(k["tokens"]) == 3
    assert lp["token_logprobs"][5:] == pytest.approx(k["token_logprobs"], abs=1e-5)


def test_prompt_logprobs_on_both_endpoints(served):
    c, asked, tok = served
    j = _post(c, "/v1/completions", prompt=PROMPT, prompt_logprobs=2, max_tokens=2,
              temperature=0, ignore_eos=True)
    ch = j["choices"][0]
    _check_plp(ch["prompt_logprobs"], PROMPT, 2)
    assert ch["logprobs"] is None
    e = _post(c, "/v1/completions", prompt=PROMPT, echo=True, logprobs=1, max_tokens=1,
              temperature=0, ignore_eos=True)["choices"][0]["logprobs"]
    got = [ch["prompt_logprobs"][i][str(PROMPT[i])]["logprob"] for i in range(1, 5)]
    assert got == pytest.approx(e["token_logprobs"][1:5], abs=1e-5)      # the two views agree
    msgs = [{"role": "user", "content": "hi there"}]
    ids = tok.encode(tok.apply_chat_template(msgs, add_generation_prompt=True))
    j = _post(c, "/v1/chat/completions", messages=msgs, prompt_logprobs=2, max_tokens=2,
              ignore_eos=True)
    _check_plp(j["choices"][0]["prompt_logprobs"], ids, 2)
    j = _post(c, "/v1/completions", prompt=PROMPT, prompt_logprobs=0, max_tokens=1)
    _check_plp(j["choices"][0]["prompt_logprobs"], PROMPT, 0)


def test_n2_computes_once(served):
    c, asked, _ = served
    del asked[:]
    j = _post(c, "/v1/completions", prompt=PROMPT, prompt_logprobs=2, n=2, max_tokens=2, seed=1,
              ignore_eos=True)
    a, b = j["choices"]
    _check_plp(a["prompt_logprobs"], PROMPT, 2)
    assert a["prompt_logprobs"] == b["prompt_logprobs"]
    assert asked == [2, None]                    # only choice 0 asked the engine


def test_batch_of_prompts(served):
    c, asked, _ = served
    del asked[:]
    other = [11, 12, 13]
    j = _post(c, "/v1/completions", prompt=[PROMPT, other], prompt_logprobs=1, n=2, echo=True,
              logprobs=1, max_tokens=2, seed=3, ignore_eos=True)
    ch = j["choices"]
    assert len(ch) == 4 and asked == [1, None, 1, None]
    for k, ids in ((0, PROMPT), (1, PROMPT), (2, other), (3, other)):
        _check_plp(ch[k]["prompt_logprobs"], ids, 1)
        lp = ch[k]["logprobs"]
        assert len(lp["tokens"]) == len(ids) + 2 and lp["token_logprobs"][0] is None
        assert lp["text_offset"][0] == 0 and "".join(lp["tokens"]) == ch[k]["text"]
    assert ch[0]["prompt_logprobs"] == ch[1]["prompt_logprobs"]
    assert ch[2]["prompt_logprobs"] == ch[3]["prompt_logprobs"] != ch[0]["prompt_logprobs"]
    single = _post(c, "/v1/completions", prompt=other, prompt_logprobs=1, max_tokens=1)
    a, b = single["choices"][0]["prompt_logprobs"], ch[2]["prompt_logprobs"]
    for x, y, t in zip(a[1:], b[1:], other[1:]):
        assert x[str(t)]["logprob"] == pytest.approx(y[str(t)]["logprob"], abs=1e-5)


def test_stream_first_chunk_carries_them(served):
    c, _, _ = served
    for path, body in (("/v1/completions", {"prompt": PROMPT}),
                       ("/v1/chat/completions", {"messages": [{"role": "user", "content": "hi"}]})):
        for n in (1, 2):
            with c.stream("POST", path, json=dict(body, prompt_logprobs=1, n=n, max_tokens=3,
                                                  stream=True, ignore_eos=True)) as s:
                lines = [l for l in s.iter_lines() if l]
            assert lines[-1] == "data: [DONE]"
            chunks = [json.loads(l[6:])["choices"][0] for l in lines[:-1]]
            for i in range(n):
                mine = [ch for ch in chunks if ch["index"] == i]
                assert isinstance(mine[0].get("prompt_logprobs"), list)
                assert mine[0]["prompt_logprobs"][0] is None
                assert all("prompt_logprobs" not in ch for ch in mine[1:])


def test_out_of_range_is_400(served):
    c, _, _ = served
    for bad in (99, -1):
        assert c.post("/v1/completions", json={"prompt": PROMPT, "prompt_logprobs": bad,
                                               "max_tokens": 1}).status_code == 400
        assert c.post("/v1/chat/completions", json={
            "messages": [{"role": "user", "content": "x"}], "prompt_logprobs": bad,
            "max_tokens": 1}).status_code == 400


def test_requests_without_the_feature_are_unchanged(served):
    c, asked, _ = served
    del asked[:]
    j = _post(c, "/v1/completions", prompt=PROMPT, max_tokens=3, logprobs=1, temperature=0,
              ignore_eos=True)
    ch = j["choices"][0]
    assert set(ch) == {"index", "text", "logprobs", "finish_reason"}
    assert len(ch["logprobs"]["tokens"]) == 3 and ch["logprobs"]["text_offset"][0] == 0
    e = _post(c, "/v1/completions", prompt=PROMPT, max_tokens=3, echo=True, temperature=0,
              ignore_eos=True)["choices"][0]
    assert set(e) == {"index", "text", "logprobs", "finish_reason"} and e["logprobs"] is None
    assert e["text"].endswith(ch["text"]) and len(e["text"]) > len(ch["text"])
    m = _post(c, "/v1/chat/completions", messages=[{"role": "user", "content": "hi"}],
              max_tokens=2)["choices"][0]
    assert set(m) == {"index", "message", "logprobs", "finish_reason"}
    assert asked == [None, None, None]
