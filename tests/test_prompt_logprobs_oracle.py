"""ops/reference.py's K15 prompt logprobs (the CPU path) against the float64 oracle
(tests/prompt_logprobs_oracle.py), on exactly the inputs of tests/test_prompt_logprobs_gpu.py:
every row of every case is judged, ids exactly, values within the oracle's bound.
"""
import numpy as np
import pytest
import torch

import prompt_logprobs_oracle as po
from kubernetes_gpu_cluster_amd import ops
from kubernetes_gpu_cluster_amd.ops import reference as ref


def test_oracle_on_a_hand_row():
    x = np.array([[1.0, 3.0, -0.0, 3.0, 0.0, -np.inf]])
    a = po.oracle(x, [2], 8)
    assert a.ids[0].tolist() == [1, 3, 0, 2, 4, 5, -1, -1]      # ties by id; -0.0 == +0.0
    lse = np.log(np.exp(1) + 2 * np.exp(3) + 2)
    assert abs(a.lse[0] - lse) < 1e-12 and abs(a.tok[0] + lse) < 1e-12
    assert a.vals[0, 5] == -np.inf and a.vals[0, 6] == -np.inf
    assert po.oracle(x, [5], 0).tok[0] == -np.inf                # target on a -inf column
    assert po.oracle(x, [7], 1, col0=4).tval[0] == 3.0           # global ids


@pytest.mark.parametrize("name", po.CASE_NAMES)
def test_reference_matches_oracle(name):
    c, ans = po.case(name), po.answer(name)
    for k in po.KS:
        tok, top, ids = ops.prompt_logprobs(c.logits, c.targets, k)
        assert tok.dtype == torch.float32 and ids.dtype == torch.int32 and ids.shape == (len(tok), k)
        po.check(ans, k, tok.numpy(), top.numpy(), ids.numpy(), f"{name} k={k}")


@pytest.mark.parametrize("name", [n for n in po.CASE_NAMES
                                  if ("R3-" in n and "V50257" not in n) or "R17-V1000" in n]
                         + ["bf16-R3-V50257", "f16-R3-V50257-offset"])
@pytest.mark.parametrize("nshard", [2, 3, 8])
def test_reference_shards_merge(name, nshard):
    """Per-shard records (one shard of padding only among them), sliced differently per
    shard, merged once; and merged per shard to one record first, as a TP rank does."""
    c, ans = po.case(name), po.answer(name)
    for k in (0, 5, 20):
        recs, ones = [], []
        for i, (t, off, nc) in enumerate(c.shards(nshard, "cpu")):
            r = ops.prompt_logprobs_partial(t, c.targets, off, nc, k, splits=1 + i % 3)
            recs.append(r)
            ones.append(ops.prompt_logprobs_merge(r, k, as_record=True)[:, None])
        for what, rec in (("slices", torch.cat(recs, 1)), ("records", torch.cat(ones, 1))):
            tok, top, ids = ops.prompt_logprobs_merge(rec, k)
            po.check(ans, k, tok.numpy(), top.numpy(), ids.numpy(), f"{name} x{nshard} {what} k={k}")


def test_empty_records_give_no_nan():
    rec = ref.prompt_logprobs_partial(torch.zeros(2, 4), torch.tensor([0, 1]), 0, 0, 3, 2)
    assert rec[:, :, 0].eq(float("-inf")).all() and rec[:, :, 1].eq(0).all()
    tok, top, ids = ref.prompt_logprobs_merge(rec, 3)
    assert tok.eq(float("-inf")).all() and top.eq(float("-inf")).all() and ids.eq(-1).all()


def test_k_range():
    with pytest.raises(ValueError):
        ops.prompt_logprobs(torch.zeros(1, 4), torch.tensor([0]), 21)
