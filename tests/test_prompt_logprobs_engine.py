"""Prompt logprobs through the engine (CPU, float32 tiny-llama): chunked prefill, the model's
own log-softmax, prefix cache, recompute preemption, async == sync, PP refusal, TP = 2."""
import dataclasses

import pytest
import torch

from kubernetes_gpu_cluster_amd.engine.sequence import SamplingParams
from kubernetes_gpu_cluster_amd.models import PRESETS

K = 3


def _llm(**kw):
    from kubernetes_gpu_cluster_amd.engine.llm_engine import LLM
    base = dict(device="cpu", dtype="float32", random_init=True, max_model_len=128,
                max_num_seqs=4, max_num_batched_tokens=128, seed=1, block_size=16,
                num_gpu_blocks_override=64)
    base.update(kw)
    return LLM("tiny-llama", **base)


def _prompt(n=70, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(3, PRESETS["tiny-llama"].vocab_size, (n,), generator=g).tolist()


def _sp(**kw):
    base = dict(temperature=0, max_tokens=3, ignore_eos=True, prompt_logprobs=K)
    base.update(kw)
    return SamplingParams(**base)


def _check_shape(plp, prompt, k=K):
    assert len(plp) == len(prompt) and plp[0] is None
    for j in range(1, len(prompt)):
        tok, lp, top = plp[j]
        assert tok == prompt[j] and lp <= 0 and len(top) == k
        assert all(v <= 0 for _, v in top)
        assert [v for _, v in top] == sorted((v for _, v in top), reverse=True)


def _close(a, b, tol):
    assert len(a) == len(b) and a[0] is None and b[0] is None
    for x, y in zip(a[1:], b[1:]):
        assert x[0] == y[0] and abs(x[1] - y[1]) <= tol
        assert [i for i, _ in x[2]] == [i for i, _ in y[2]]
        assert all(abs(u - v) <= tol for (_, u), (_, v) in zip(x[2], y[2]))


@pytest.fixture(scope="module")
def one_chunk():
    """The 70-token prompt in one prefill chunk: (prompt, prompt_logprobs, engine's model)."""
    llm = _llm()
    prompt = _prompt()
    out = llm.generate([prompt], _sp())[0]
    model = llm.engine.executor.runner.model
    llm.shutdown()
    return prompt, out.prompt_logprobs, model, out.output_token_ids


def test_chunked_prefill_matches_one_chunk(one_chunk):
    prompt, ref, _, toks = one_chunk
    _check_shape(ref, prompt)
    llm = _llm(max_num_batched_tokens=24)               # 70 tokens: 3 chunks
    out = llm.generate([prompt], _sp())[0]
    st = llm.engine.executor.runner.stats
    llm.shutdown()
    assert st["eager_steps"] >= 3 + 2 and st["plp_rows"] == len(prompt) - 1
    assert out.output_token_ids == toks
    _check_shape(out.prompt_logprobs, prompt)
    _close(out.prompt_logprobs, ref, 1e-5)


def test_row_cap_splits_the_lm_head_calls(one_chunk, monkeypatch):
    """KGC_PLP_LOGITS_MB bounds the logits held at once: 5 rows of 1024 fp32 columns here,
    so the 69 rows of the one-chunk prefill take 14 LM-head calls -- same values."""
    prompt, ref, _, _ = one_chunk
    monkeypatch.setenv("KGC_PLP_LOGITS_MB", "0.02")
    llm = _llm()
    runner = llm.engine.executor.runner
    assert runner.plp_rows == 5
    calls = []
    head = runner.model.compute_logits
    monkeypatch.setattr(runner.model, "compute_logits",
                        lambda h, gather=True: calls.append(h.shape[0]) or head(h, gather))
    out = llm.generate([prompt], _sp(max_tokens=1))[0]
    llm.shutdown()
    assert calls == [5] * 13 + [4, 1]                     # ... and the sampled row
    _close(out.prompt_logprobs, ref, 1e-6)


def test_matches_log_softmax_of_the_models_logits(one_chunk):
    from test_model_parity import _engine_logits
    from kubernetes_gpu_cluster_amd.engine.model_runner import ModelRunner
    from kubernetes_gpu_cluster_amd.parallel.state import ParallelState, set_state
    prompt, plp, model, _ = one_chunk
    set_state(ParallelState())
    cfg = PRESETS["tiny-llama"]
    runner = ModelRunner(model, cfg, torch.float32, torch.device("cpu"), block_size=16,
                         max_model_len=256, max_num_seqs=4, token_budget=128, enforce_eager=True)
    runner.init_kv_cache(48)
    lsm = torch.log_softmax(_engine_logits(model, runner, prompt, [len(prompt)], []).double(), -1)
    for j in range(1, len(prompt)):
        tok, lp, top = plp[j]
        assert abs(lsm[j - 1, tok].item() - lp) <= 1e-4
        want = torch.sort(lsm[j - 1], descending=True, stable=True)
        assert [i for i, _ in top] == want.indices[:K].tolist()
        assert all(abs(v - w) <= 1e-4 for (_, v), w in zip(top, want.values[:K].tolist()))


def test_k0_and_unflagged_requests(one_chunk):
    prompt, ref, _, _ = one_chunk
    llm = _llm()
    outs = llm.generate([prompt, prompt[:9], [7]],
                        [_sp(prompt_logprobs=0), _sp(prompt_logprobs=None), _sp()])
    llm.shutdown()
    _check_shape(outs[0].prompt_logprobs, prompt, 0)
    assert all(abs(a[1] - b[1]) <= 1e-5 for a, b in zip(outs[0].prompt_logprobs[1:], ref[1:]))
    assert outs[1].prompt_logprobs is None
    assert outs[2].prompt_logprobs == [None]               # a one-token prompt


def test_prefix_cache_is_bypassed_and_still_published(one_chunk):
    prompt, ref, _, _ = one_chunk
    llm = _llm(enable_prefix_caching=True)
    bm = llm.engine.bm
    llm.generate([prompt], _sp(prompt_logprobs=None))
    h0 = bm.hit_tokens
    out = llm.generate([prompt], _sp())[0]                   # flagged: every position computed
    assert bm.hit_tokens == h0
    _close(out.prompt_logprobs, ref, 1e-5)
    llm.generate([prompt], _sp(prompt_logprobs=None))        # unflagged: hits again
    assert bm.hit_tokens >= h0 + 64
    llm.shutdown()


def test_recompute_preemption_reports_each_position_once(monkeypatch):
    monkeypatch.setenv("KGC_DEBUG", "1")
    prompts = [[5 + i, 6, 7, 8, 9, 10, 11] * 3 for i in range(4)]
    sp = _sp(max_tokens=20)
    ample = _llm(max_model_len=64, max_num_batched_tokens=48)
    ref = ample.generate(prompts, sp)
    rows_ref = ample.engine.executor.runner.stats["plp_rows"]
    ample.shutdown()
    tight = _llm(num_gpu_blocks_override=6, max_model_len=64, max_num_batched_tokens=48)
    got = tight.generate(prompts, sp)
    npre = tight.engine.scheduler.num_preemptions
    rows = tight.engine.executor.runner.stats["plp_rows"]
    tight.shutdown()
    assert npre > 0
    assert rows == rows_ref == sum(len(p) - 1 for p in prompts)      # none requested twice
    for p, a, b in zip(prompts, got, ref):
        assert a.output_token_ids == b.output_token_ids
        _check_shape(a.prompt_logprobs, p)
        _close(a.prompt_logprobs, b.prompt_logprobs, 1e-5)


def test_async_equals_sync():
    prompts = [_prompt(40, 1), [9] * 30, [11, 12]]
    sps = [_sp(temperature=0.8, seed=s, max_tokens=5, prompt_logprobs=k)
           for s, k in ((1, 2), (2, 0), (3, 5))]
    outs = []
    for async_output in (True, False):
        llm = _llm(async_output=async_output, max_num_batched_tokens=32)
        assert llm.engine.async_mode == async_output
        outs.append(llm.generate(prompts, sps))
        llm.shutdown()
    for p, sp, a, b in zip(prompts, sps, *outs):
        assert a.output_token_ids == b.output_token_ids
        _check_shape(a.prompt_logprobs, p, sp.prompt_logprobs)
        _close(a.prompt_logprobs, b.prompt_logprobs, 1e-6)


def test_params_range():
    for bad in (-1, 21):
        with pytest.raises(ValueError):
            SamplingParams(prompt_logprobs=bad)
    assert SamplingParams(prompt_logprobs=20).prompt_logprobs == 20


def test_pp2_rejects_prompt_logprobs():
    llm = _llm(pipeline_parallel_size=2, max_num_batched_tokens=64, num_gpu_blocks_override=32)
    try:
        with pytest.raises(ValueError, match="prompt_logprobs are not supported with pipeline"):
            llm.engine.add_request([5, 6, 7], SamplingParams(max_tokens=2, prompt_logprobs=1))
        outs = llm.generate([[5, 6, 7]], _sp(prompt_logprobs=None))
        assert len(outs[0].output_token_ids) == 3 and outs[0].prompt_logprobs is None
    finally:
        llm.shutdown()


def test_fake_engine_accepts_the_field():
    from kubernetes_gpu_cluster_amd.engine.fake import FakeEngine
    from kubernetes_gpu_cluster_amd.engine.config import EngineConfig
    eng = FakeEngine(EngineConfig(model="tiny-llama", device="cpu"), timing=(0.0, 0.0, 0.0))
    eng.add_request([1, 2, 3], SamplingParams(max_tokens=2, prompt_logprobs=2), request_id="a")
    outs = []
    while eng.has_unfinished():
        outs += eng.step()
    assert outs and all(o.prompt_logprobs is None for o in outs)


# ---------------------------------------------------------------------------- TP = 2 (gloo)
def _tp_run(rank, tp, vocab):
    from kubernetes_gpu_cluster_amd.engine.block_manager import BlockManager
    from kubernetes_gpu_cluster_amd.engine.model_runner import ModelRunner
    from kubernetes_gpu_cluster_amd.engine.sequence import Sequence
    from kubernetes_gpu_cluster_amd.models import build_model, full_state_dict_random
    from kubernetes_gpu_cluster_amd.parallel.state import destroy_parallel, init_parallel
    init_parallel(tp, 1, backend="gloo", device=torch.device("cpu"))
    cfg = dataclasses.replace(PRESETS["tiny-llama"], vocab_size=vocab)
    model = build_model(cfg, torch.float32, torch.device("cpu"))
    model.load_weights(full_state_dict_random(cfg, seed=3, std=0.05).items())
    runner = ModelRunner(model, cfg, torch.float32, torch.device("cpu"), 16, 256, 4, 128, True)
    runner.init_kv_cache(48)
    g = torch.Generator().manual_seed(0)
    prompt = torch.randint(3, vocab, (29,), generator=g).tolist()
    bm = BlockManager(48, 16, 4, runner.max_blocks)
    seq = Sequence("0", prompt, SamplingParams(temperature=0, prompt_logprobs=4))
    got = []
    for n in (13, 16):
        bm.allocate(seq, seq.num_computed + n)
        plan, _ = runner.build_plan([(seq, n)], [], bm.table)
        runner.run(plan)
        got.append(runner.take_prompt_logprobs())
        seq.num_computed += n
    shard = (runner.plp_shard, runner.plp_off, runner.plp_cols, runner.stats["tp_plp_bytes"])
    destroy_parallel()
    return [torch.cat(x) for x in zip(*got)], shard


@pytest.mark.parametrize("vocab", [1001, 61])
def test_tp2_matches_tp1(vocab):
    """vocab 1001: rank 1's shard is part padding; vocab 61: padding only (empty records).
    Each rank contributes one (3 + 2k)-word record per row, never logits."""
    from test_distributed import spawn
    (ref, s1), = spawn(_tp_run, 1, 1, vocab).values()
    got = spawn(_tp_run, 2, 2, vocab)
    assert s1 == (False, 0, vocab, 0) and ref[0].shape == (28,)
    per = {1001: 512, 61: 64}[vocab]
    for r in range(2):
        out, (shard, off, cols, nbytes) = got[r]
        assert shard and off == r * per and cols == max(0, min(per, vocab - r * per))
        assert nbytes == 28 * (3 + 2 * 4) * 4
        assert torch.equal(out[2], ref[2])
        torch.testing.assert_close(out[0], ref[0], atol=1e-5, rtol=0)
        torch.testing.assert_close(out[1], ref[1], atol=1e-5, rtol=0)


def test_multiproc_tp2_engine_matches_tp1(tmp_path):
    """The whole engine at TP = 2 (spawned rank, plan blobs broadcast over gloo): the worker
    rank builds its row list from the blob it received, and the driver's values equal
    TP = 1's."""
    from test_distributed import _write_hf_dir
    from kubernetes_gpu_cluster_amd.engine.llm_engine import LLM
    d = str(tmp_path / "m")
    _write_hf_dir(d, "tiny-llama")
    prompts = [_prompt(40, 2), [5, 6, 7] * 9, [9]]
    sps = [_sp(prompt_logprobs=k) for k in (2, None, 4)]
    outs = {}
    for tp in (1, 2):
        llm = LLM(d, device="cpu", dtype="float32", tensor_parallel_size=tp, max_model_len=256,
                  max_num_seqs=4, max_num_batched_tokens=24, num_gpu_blocks_override=64)
        outs[tp] = llm.generate(prompts, sps)
        llm.shutdown()
    for p, sp, a, b in zip(prompts, sps, outs[2], outs[1]):
        assert a.output_token_ids == b.output_token_ids
        if sp.prompt_logprobs is None:
            assert a.prompt_logprobs is None and b.prompt_logprobs is None
        else:
            _check_shape(a.prompt_logprobs, p, sp.prompt_logprobs)
            _close(a.prompt_logprobs, b.prompt_logprobs, 1e-5)
