"""K15 prompt logprobs on the GPU, every row judged by the float64 oracle
(tests/prompt_logprobs_oracle.py): top-k ids exactly, values within
1e-4 + 2^-20 max(|t|, |lse|).

The matrix crosses R in {1, 3, 17} with V in {8, 1000, 4104, 50257} (and one row at 128256),
bf16 / f16 / fp32 and k in {0, 1, 5, 20} (V = 8 with k = 20: the padded tail), over input
families: gaussian at scales 1 and 10, peaked, flat (every value tied), integer-quantised,
-inf-masked down to one finite column, the target on a -inf column, signed zeros at the k
boundary, magnitudes near the dtype's maximum.  With the kernel's own split (32 / 31
workgroups per row at these R) V = 8 and 1000 leave workgroups an empty slice or one shorter
than a 16-byte vector; ``splits`` = the fewest slices that fit the LDS stage gives whole-row
and full-stage workgroups.  "wide" and "offset" rows have a stride above V and start at an
odd element.

Largest error seen on an MI355X over the whole file: 1.97e-6 on the rows with ordinary
magnitudes (2 % of the 1e-4 bound) and 0.107 of the bound at worst, on the f16 rows near
+-6e4, where the error is the fp32 rounding of t - lse (2.4e-3 against a bound of 0.057).
"""
import pytest
import torch

import prompt_logprobs_oracle as po
from kubernetes_gpu_cluster_amd import ops

pytestmark = pytest.mark.gpu

_seen = {"err": 0.0, "share": 0.0}       # err: over the rows with |logit| <= 100


def _judge(ans, k, out, what):
    tok, top, ids = (t.cpu().numpy() for t in out)
    e, share = po.check(ans, k, tok, top, ids, what)
    if e < 1e-3:               # the "huge" rows err by ulps of 6e4 / 1e38: see the share
        _seen["err"] = max(_seen["err"], e)
    _seen["share"] = max(_seen["share"], share)
    print(f"{what}: max error {e:.3e}, {share:.3f} of its bound "
          f"(file so far {_seen['err']:.3e}, {_seen['share']:.3f})")


@pytest.mark.parametrize("name", po.CASE_NAMES)
def test_kernel_matrix(gpu, name):
    c, ans = po.case(name), po.answer(name)
    x, tg = c.place(gpu), c.targets.to(gpu)
    V = x.shape[1]
    fewest = -(-V // 8192)
    for k in po.KS:
        _judge(ans, k, ops.prompt_logprobs(x, tg, k), f"{name} k={k}")
        rec = ops.prompt_logprobs_partial(x, tg, 0, V, k, splits=fewest)
        assert rec.shape == (x.shape[0], fewest, 3 + 2 * k)
        _judge(ans, k, ops.prompt_logprobs_merge(rec, k), f"{name} k={k} splits={fewest}")


@pytest.mark.parametrize("name", [n for n in po.CASE_NAMES if "R17-" in n or "V128256" in n
                                  or n.startswith("bf16-R3-V50257-")])
@pytest.mark.parametrize("nshard", [2, 3, 8])
def test_shards_merge(gpu, name, nshard):
    """Column shards with vocab_off / ncols (one of padding only): partial per shard, one
    merge -- and each shard merged to one record first, as a TP rank does before the
    all-gather.  Ids equal the unsharded call's, values stay within the bound."""
    c, ans = po.case(name), po.answer(name)
    tg = c.targets.to(gpu)
    for k in (0, 5, 20):
        whole = ops.prompt_logprobs(c.place(gpu), tg, k)
        recs, ones = [], []
        for t, off, nc in c.shards(nshard, gpu):
            r = ops.prompt_logprobs_partial(t, tg, off, nc, k)
            recs.append(r)
            ones.append(ops.prompt_logprobs_merge(r, k, as_record=True)[:, None])
        for what, rec in (("slices", torch.cat(recs, 1)), ("records", torch.cat(ones, 1))):
            out = ops.prompt_logprobs_merge(rec, k)
            assert torch.equal(out[2], whole[2])
            _judge(ans, k, out, f"{name} x{nshard} {what} k={k}")


def test_empty_shard_alone(gpu):
    """ncols = 0 everywhere: empty records, and -inf (never NaN) out of the merge."""
    x = torch.full((3, 16), 60.0, dtype=torch.bfloat16, device=gpu)
    rec = ops.prompt_logprobs_partial(x, torch.tensor([0, 5, 15], device=gpu), 32, 0, 4)
    assert rec[:, :, 0].eq(float("-inf")).all() and rec[:, :, 1].eq(0).all()
    tok, top, ids = ops.prompt_logprobs_merge(rec, 4)
    assert tok.eq(float("-inf")).all() and top.eq(float("-inf")).all() and ids.eq(-1).all()


def test_no_row_sized_intermediate(gpu):
    """Around one call at R = 64, V = 50257 the allocator's peak grows by the records and
    the outputs only (each rounded up to the allocator's 512-byte granule) -- far below
    R * V * 4 bytes."""
    R, V, k = 64, 50257, 20
    x = torch.randn(R, V, device=gpu).to(torch.bfloat16)
    tg = torch.randint(V, (R,), device=gpu)
    S = int(torch.ops.kgc.plp_splits(R, V))
    up = lambda n: -(-n // 512) * 512   # noqa: E731
    limit = up(R * S * (3 + 2 * k) * 4) + up(R * 4) + 2 * up(R * k * 4)
    assert limit < R * V * 4 // 16
    ops.prompt_logprobs(x, tg, k)                 # library load, first-call allocations
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = ops.prompt_logprobs(x, tg, k)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - base
    assert grew <= limit, (grew, limit)
    a = po.oracle(x.double().cpu().numpy(), tg.cpu().numpy(), k)
    _judge(a, k, out, "R64-V50257")


def test_argument_checks(gpu):
    x = torch.zeros(2, 64, dtype=torch.bfloat16, device=gpu)
    tg = torch.zeros(2, dtype=torch.int64, device=gpu)
    with pytest.raises(ValueError):
        ops.prompt_logprobs(x, tg, 21)
    with pytest.raises(RuntimeError):
        ops.prompt_logprobs_partial(x, tg, 0, 65, 1)             # ncols beyond the shard
    with pytest.raises(RuntimeError):
        big = torch.zeros(1, 20000, dtype=torch.bfloat16, device=gpu)
        ops.prompt_logprobs_partial(big, tg[:1], 0, 20000, 1, splits=2)   # slice > LDS stage


# ---------------------------------------------------------------------------- engine
@pytest.mark.parametrize("graphs", [False, True])
def test_engine_prompt_logprobs_match_hf(gpu, tmp_path, graphs):
    """bf16 tiny-llama, the 70-token prompt of test_gpu_logits_match_hf in prefill chunks of
    33 and 37 through the engine's runner: prompt_logprobs against log_softmax of the HF fp32
    logits within 2 (0.03 scale + 1e-3) -- twice the per-logit bound that test accepts, since
    a logit error of e moves a log-softmax value by at most 2e.  With graphs on, the decode
    steps behind the prefill still replay them."""
    import json
    from safetensors.torch import save_file
    from kubernetes_gpu_cluster_amd.engine.llm_engine import LLM
    from kubernetes_gpu_cluster_amd.engine.sequence import SamplingParams, Sequence
    from kubernetes_gpu_cluster_amd.models import PRESETS, full_state_dict_random
    from test_model_parity import _hf_model
    cfg = PRESETS["tiny-llama"]
    sd = full_state_dict_random(cfg, seed=2, std=0.05)
    hf, _ = _hf_model(cfg, sd)
    save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / "model.safetensors"))
    json.dump({"model_type": "llama", "hidden_size": cfg.hidden_size,
               "num_hidden_layers": cfg.num_layers, "num_attention_heads": cfg.num_heads,
               "num_key_value_heads": cfg.num_kv_heads, "head_dim": cfg.head_dim,
               "intermediate_size": cfg.intermediate_size, "vocab_size": cfg.vocab_size,
               "max_position_embeddings": 512, "rope_theta": cfg.rope_theta,
               "rms_norm_eps": cfg.rms_eps, "eos_token_id": 2, "bos_token_id": 1},
              open(tmp_path / "config.json", "w"))
    g = torch.Generator().manual_seed(0)
    prompt = torch.randint(3, cfg.vocab_size, (70,), generator=g).tolist()
    with torch.no_grad():
        ref = torch.log_softmax(hf(torch.tensor([prompt])).logits[0].float(), -1)
        scale = hf(torch.tensor([prompt])).logits[0].float().abs().max().item()
    tol = 2 * (0.03 * scale + 1e-3)
    k = 5
    llm = LLM(str(tmp_path), max_model_len=256, max_num_seqs=4, max_num_batched_tokens=128,
              num_gpu_blocks_override=48, block_size=16, cuda_graph_max_bs=4,
              enforce_eager=not graphs)
    try:
        runner, bm = llm.engine.executor.runner, llm.engine.bm
        seq = Sequence("plp", prompt, SamplingParams(temperature=0, prompt_logprobs=k))
        got = []
        for n in (33, 37):
            bm.allocate(seq, seq.num_computed + n)
            plan, _ = runner.build_plan([(seq, n)], [], bm.table)
            res = runner.run(plan)
            got.append(runner.take_prompt_logprobs())
            seq.num_computed += n
        for _ in range(3):                                  # decode steps behind the prefill
            seq.output_token_ids.append(int(res[0]))
            bm.allocate(seq, seq.num_computed + 1)
            plan, _ = runner.build_plan([], [seq], bm.table)
            res = runner.run(plan)
            seq.num_computed += 1
        torch.cuda.synchronize()
        st = dict(runner.stats)
    finally:
        llm.shutdown()
    assert (st["graph_steps"] == 3) if graphs else (st["graph_steps"] == 0), st
    assert st["plp_rows"] == 69
    tok, top, ids = (torch.cat(x) for x in zip(*got))
    assert tok.shape == (69,) and top.shape == (69, k) and ids.shape == (69, k)
    want = ref[torch.arange(69), torch.tensor(prompt[1:])]
    err = (tok - want).abs().max().item()
    print(f"graphs={graphs}: token logprob error {err:.4f} (tolerance {tol:.4f}, scale {scale:.3f})")
    assert err <= tol
    # each reported alternative carries its own log-softmax value (bf16 may reorder near-ties)
    alt = ref[:69].gather(1, ids.long())
    assert (top - alt).abs().max().item() <= tol
    assert (top[:, :-1] >= top[:, 1:]).all() and (top <= 0).all()
    assert (top[:, 0] >= ref[:69].max(-1).values - tol).all()
